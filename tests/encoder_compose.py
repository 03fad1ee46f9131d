"""A second implementation of the encoder recipes of include/mer_hip.h, issued from Python over the op-level ABI.

mertools_amd/csrc/encoders.cpp turns a checkpoint into a fixed sequence of op-level calls (mer_gemm16, mer_seq_bias, mer_layernorm,
the attention kernels, ...).  The ops are pinned one by one against fp64 references elsewhere in this suite, and the project claims
that their dispatch variants (GEMM tiles / loaders / persistent kernel, LayerNorm variants) agree bit for bit and that a row's result
does not depend on its batch.  So the same sequence issued from here, on operands built independently from the state dict, must give
the SAME BITS as the library's forward: any difference is an orchestration defect (an offset into a fused plane, a table built with
the wrong n_first, a lost valid_rows pointer, a silent one-pass fall-back) or an undocumented dependence.

Rules of this file:
  * every operand is built here from the state dict (split16_host, mx_pack, w_block_pack, w_block_pack_p); nothing is borrowed from
    a model object;
  * where the library addresses a SUB-RANGE of a fused plane (the V rows under mx_skip bit 0 with passes == 4, the K | V rows and
    the Q rows of the CLS-only block) the sub-matrix is packed on its own and passed un-offset: the comparison does not share the
    offset arithmetic under test;
  * torch moves memory (views, allocation) only; every number comes out of a kernel of libmer_hip.so;
  * `mis` (a set of names) mis-composes on purpose, in Python only and with every read in bounds: the negative controls of
    tests/test_encoder_compose_gpu.py.

`expected_path` restates tf_forward's dispatch as a pure predicate (no GPU): tests/test_encoder_compose_cpu.py asserts what the
case table reaches through it.  `block` / `cls_block` record the path they really take, from the operands they really hold, in
Layer.trace; the GPU tests require trace == expected_path for every block they run, so the predicate cannot drift from the
composition, and the composition is held to the library by its bits.

hubert_front's pass-code decisions (the projection's table, the positional conv's 4 / 5 -> 2) follow the text at
mer_hubert_config.conv_passes.
"""
from types import SimpleNamespace

import torch

# preset -> (conv-stack passes, block passes, fp32 attention under passes == 6): README.md "precision presets" / DESIGN.md §4
PRESETS = {"fast": (1, 1, 0), "balanced": (2, 2, 0), "mx": (4, 4, 0), "mean": (4, 5, 0), "mean_conv3": (3, 5, 0), "mean_a2": (4, 6, 0),
           "a2_conv3": (3, 6, 0), "accurate": (3, 3, 0),
           "mean_a2f": (4, 6, 1), "x3_conv4": (4, 3, 0), "mean_all": (5, 5, 0), "mean_conv": (5, 2, 0)}
PUBLIC_PRESETS = ("fast", "balanced", "mx", "mean", "mean_conv3", "mean_a2", "a2_conv3", "accurate")
MISCOMPOSE = ("drop_table", "n_first0", "no_valid", "v_from_q")
# (+ "two_pass_for_table": the table replaced by an exact second pass over the `lo` plane — a MORE accurate GEMM, not the recipe's;
#    "kv_mx": the CLS-only block's K | V GEMM given an MX plane although hidden % 256 != 0 — against the header's tile rule)


def tf_cfg(D, F, layers, *, pre_ln, act, eps, dtype, preset, mx_skip, swiglu=False, gated=False):
    """The fields of mer_tf_config the recipe reads."""
    _, passes, a32 = PRESETS[preset]
    return SimpleNamespace(D=D, H=D // 64, F=F, layers=layers, pre_ln=bool(pre_ln), act=act, eps=eps, dtype=dtype, passes=passes,
                           mx_skip=mx_skip, attn_f32=a32, swiglu=bool(swiglu), gated=bool(gated), conv_passes=PRESETS[preset][0])


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch of one block, restated from the header (pure Python)
# ------------------------------------------------------------------------------------------------------------------------------
def mx_plane_exists(c, K):
    """A weight [N, K] carries an MX residual plane iff the preset is MX-corrected, the planes are f16 and K % 128 == 0 (mer_mx_pack)."""
    return c.passes == 4 and c.dtype == "f16" and K % 128 == 0


def corr_kind(passes, *, a_lo, w_lo, w_mx, seq, dtype="f16", N=256, K=128):
    """What a GEMM issued with pass code `passes` runs: one of
      "1" / "2" / "3"   plain one-, two-, three-pass;   "mx" the MX kernel;   "2(mx)" passes == 4 on a shape the MX kernel does not cover
      "tab1" / "tab2"   passes 5 / 6 with the per-sequence table over one / two MFMA passes;
    with the documented degradations where there is no table (no sequence structure / no `lo` plane): 5 -> 4 -> 2, 6 -> 3."""
    if passes in (5, 6):
        a2 = passes == 6 and a_lo
        if seq and w_lo and N % 8 == 0 and K % 8 == 0:
            return "tab2" if a2 else "tab1"
        passes = 3 if a2 else (4 if (w_mx or w_lo) else 1)
    if passes == 4:
        mx = w_mx and N >= 192 and dtype == "f16" and K % 128 == 0
        return "mx" if mx else "2(mx)"
    return str(passes)


def expected_path(c, *, block=0, T=64, Bseq=16, cls_only=False, score_bias=False):
    """tf_forward's dispatch for block `block` of config `c` (tf_cfg), from include/mer_hip.h:
    -> dict(qkv, attention, ffn, corr={gemm: kind}, cls_only, tiles)."""
    D, F, ps = c.D, c.F, c.passes
    lo = ps >= 2
    a_lo = ps in (3, 6)
    sel = ps in (4, 5)
    ps1 = 1 if (sel and c.mx_skip & 2) else ps
    ps2 = 1 if (sel and c.mx_skip & 4) else ps
    kw = dict(a_lo=a_lo, w_lo=lo, dtype=c.dtype)
    last = cls_only and block == c.layers - 1
    out = dict(cls_only=bool(last), tiles=None, corr={})
    if last:
        tiles = D % 256 == 0
        out["tiles"] = tiles
        out["qkv"] = "cls: kv + q"
        out["attention"] = "cls"
        out["ffn"] = "plain"
        out["corr"]["kv"] = corr_kind(ps, w_mx=mx_plane_exists(c, D) and tiles, seq=True, N=2 * D, K=D, **kw)
        out["corr"]["q"] = corr_kind(ps, w_mx=False, seq=True, N=D, K=D, **kw)
        out["corr"]["wo"] = corr_kind(ps, w_mx=mx_plane_exists(c, D), seq=True, N=D, K=D, **kw)
        out["corr"]["fc1"] = corr_kind(ps1, w_mx=mx_plane_exists(c, D), seq=True, N=F, K=D, **kw)
        out["corr"]["fc2"] = corr_kind(ps2, w_mx=mx_plane_exists(c, F), seq=True, N=D, K=F, **kw)
        return out
    f32attn = (ps == 3 or (ps == 6 and c.attn_f32)) and not score_bias
    if ps == 4 and (c.mx_skip & 1) and (2 * D) % 256 == 0 and mx_plane_exists(c, D):
        out["qkv"] = "split: qk one pass + v"
        out["corr"]["qk"] = "1"
        out["corr"]["v"] = corr_kind(ps, w_mx=True, seq=True, N=D, K=D, **kw)
    else:
        out["qkv"] = "fused fp32" if f32attn else "fused"
        out["corr"]["qkv"] = corr_kind(ps, w_mx=mx_plane_exists(c, D), seq=True, N=3 * D, K=D, **kw)
        if ps in (5, 6):
            out["corr"]["qkv"] += " n_first=%d" % (2 * D if (c.mx_skip & 1) else 0)
    out["attention"] = "f32" if f32attn else ("bias+gate" if (score_bias and c.gated) else ("bias" if score_bias else "plain"))
    out["ffn"] = "swiglu" if c.swiglu else "plain"
    out["corr"]["wo"] = corr_kind(ps, w_mx=mx_plane_exists(c, D), seq=True, N=D, K=D, **kw)
    out["corr"]["fc1"] = corr_kind(ps1, w_mx=mx_plane_exists(c, D), seq=True, N=(2 * F if c.swiglu else F), K=D, **kw)
    out["corr"]["fc2"] = corr_kind(ps2, w_mx=mx_plane_exists(c, F), seq=True, N=D, K=F, **kw)
    return out


def vit_cls_only(c, tokens, *, variant=0, tokens_out=False, score_bias=False):
    """The CLS-only last block runs for CLIP towers (variant 0) whose caller reads image features only: pre-LN, plain FFN, no score
    bias, at most 584 tokens, 16-bit attention (not passes == 3, not passes == 6 with attn_f32)."""
    return (variant == 0 and c.pre_ln and not c.swiglu and not c.gated and tokens <= 584 and c.passes != 3
            and not (c.passes == 6 and c.attn_f32) and not tokens_out and not score_bias)


# ------------------------------------------------------------------------------------------------------------------------------
# operands and raw calls
# ------------------------------------------------------------------------------------------------------------------------------
def _ops():
    from mertools_amd import _lib, ops
    return _lib, ops


def pack(w, *, dtype, passes, dev, mx=None, blk=True):
    """The planes of one weight matrix [N, K] (host fp32) for pass code `passes`, all made here: hi (+ lo for passes >= 2), the MX
    residual plane (passes == 4, f16, K % 128 == 0; `mx=False` withholds it), the pre-blocked copies where a 256-wide kernel can
    read them (N >= 192, K % 32 == 0) and the row-permuted ones (asked for whenever the others are; the packer itself returns
    none unless N % 256 == 0)."""
    _lib, ops = _ops()
    w = w.detach().to(torch.float32).contiguous()
    N, K = w.shape
    hi_h, lo_h = ops.split16_host(w, dtype, lo=True)
    p = SimpleNamespace(N=N, K=K, hi=hi_h.contiguous().to(dev), lo=None, mx=None, hb=None, lb=None, hp=None, hq=None)
    if passes >= 2:
        p.lo = lo_h.contiguous().to(dev)
    want_mx = (passes == 4 and dtype == "f16") if mx is None else (mx and passes == 4 and dtype == "f16")
    if want_mx:
        packed = ops.mx_pack(w - hi_h.to(torch.float32))
        p.mx = packed.to(dev) if packed is not None else None
    if blk and N >= 192 and K % 32 == 0:
        p.hb = ops.w_block_pack(p.hi)
        p.lb = ops.w_block_pack(p.lo) if p.lo is not None else None
        p.hp = ops.w_block_pack_p(p.hi, 0)
        p.hq = ops.w_block_pack_p(p.hi, 1)
    return p


def pack_hi_only(wp):
    """The same weight with its hi planes alone: what a one-pass GEMM (plain, or under the correction table) is handed."""
    one = SimpleNamespace(**vars(wp))
    one.lo = one.mx = one.lb = None
    return one


def _ptr(t):
    return None if t is None else t.data_ptr()


def gemm(a_hi, a_lo, wp, *, dtype, passes, M=None, lda=None, bias=None, act=None, residual=None, c32=None, c16=None, c16_lo=None,
         seg_rows=0, arpb=0, abstride=0):
    """One mer_gemm16 on caller-owned outputs (2-D views: their row strides become the ld*)."""
    _lib, ops = _ops()
    g = _lib.GemmArgs()
    g.M = int(M if M is not None else a_hi.shape[0])
    g.N, g.K, g.dtype = wp.N, wp.K, ops.dt_code(dtype)
    g.a_hi, g.a_lo = _ptr(a_hi), _ptr(a_lo)
    g.lda = int(lda if lda is not None else a_hi.stride(0))
    g.a_rows_per_batch, g.a_batch_stride = int(arpb), int(abstride)
    g.w_hi, g.w_lo, g.ldw, g.w_mx = _ptr(wp.hi), _ptr(wp.lo), wp.K, _ptr(wp.mx)
    g.w_hi_blk, g.w_lo_blk, g.w_hi_blkp, g.w_hi_blkq = _ptr(wp.hb), _ptr(wp.lb), _ptr(wp.hp), _ptr(wp.hq)
    g.bias, g.act = _ptr(bias), ops.ACT[act]
    if seg_rows:
        g.bias_seg_rows, g.bias_ld = int(seg_rows), bias.stride(0)
    if residual is not None:
        g.residual, g.ldr = _ptr(residual), residual.stride(0)
    if c32 is not None:
        g.c32, g.ldc32 = _ptr(c32), c32.stride(0)
    if c16 is not None:
        g.c16_hi, g.c16_lo, g.ldc16 = _ptr(c16), _ptr(c16_lo), c16.stride(0)
    g.nbatch, g.nb_inner, g.passes, g.tile = 1, 1, int(passes), 0
    ops.gemm16_raw(g)


def seq_bias(a_hi, w_lo, bias, *, M, K, lda, seg_rows, valid, n_first, dtype, arpb=0, abstride=0):
    """mer_seq_bias on an A plane addressed like mer_gemm16's -> table fp32 [ceil(M / seg_rows), N]."""
    _lib, ops = _ops()
    N = w_lo.shape[0]
    nseq = (M + seg_rows - 1) // seg_rows
    dev = a_hi.device
    scratch = torch.empty(max(int(_lib.lib().mer_seq_bias_scratch_bytes(nseq, K)), 16), dtype=torch.uint8, device=dev)
    table = torch.empty((nseq, N), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mer_seq_bias(a_hi.data_ptr(), ops.dt_code(dtype), int(lda), int(arpb), int(abstride), int(M), int(K), int(seg_rows),
                                       _ptr(valid), w_lo.data_ptr(), w_lo.stride(0), _ptr(bias), N, int(n_first), scratch.data_ptr(),
                                       table.data_ptr(), N, ops.stream()), "mer_seq_bias")
    return table


def corrected_gemm(a_hi, a_lo, wp, bias, *, dtype, passes, seg_rows=0, valid=None, n_first=0, mis=(), table_lo=None, name=None, trace=None,
                   **kw):
    """mer_tf_config.passes 5 / 6 on top of the op-level ABI: mer_seq_bias over the sequences of `seg_rows` rows of the A plane
    (valid_rows = `valid`, plain bias below column n_first), then ONE pass a_hi*w_hi (5) or TWO, a_hi*w_hi + a_lo*w_hi (6, needs
    a_lo), with the table as bias.  Without sequence structure (seg_rows == 0) or a `lo` plane: 5 -> 4 (-> 2 inside mer_gemm16),
    6 -> 3.  Other pass codes go straight to mer_gemm16.  table_lo: the plane the TABLE is built from (default wp.lo).
    trace / name: records under trace[name] what this call issues, in corr_kind's words, from the operands it really holds."""
    if trace is not None:
        kind = corr_kind(passes, a_lo=a_lo is not None, w_lo=wp.lo is not None, w_mx=wp.mx is not None, seq=seg_rows > 0, dtype=dtype,
                         N=wp.N, K=wp.K)
        trace[name] = kind + (" n_first=%d" % n_first if (name == "qkv" and kind.startswith("tab")) else "")
    if passes in (5, 6):
        M = int(kw.get("M") if kw.get("M") is not None else a_hi.shape[0])
        lda = int(kw.get("lda") if kw.get("lda") is not None else a_hi.stride(0))
        a2 = passes == 6 and a_lo is not None
        ok = seg_rows > 0 and wp.lo is not None and wp.N % 8 == 0 and wp.K % 8 == 0
        if ok and "drop_table" in mis:      # the silent fall-back to ONE pass: a_hi * w_hi + the plain bias, no lo / MX plane in sight
            return gemm(a_hi, None, pack_hi_only(wp), dtype=dtype, passes=1, bias=bias, **kw)
        if ok and "two_pass_for_table" in mis:   # the weight residual through the `lo` plane itself (passes 2) instead of the table
            two = pack_hi_only(wp)
            two.lo, two.lb = wp.lo, wp.lb
            return gemm(a_hi, None, two, dtype=dtype, passes=2, bias=bias, **kw)
        if ok:
            tab = seq_bias(a_hi, table_lo if table_lo is not None else wp.lo, bias, M=M, K=wp.K, lda=lda, seg_rows=seg_rows,
                           valid=None if "no_valid" in mis else valid, n_first=n_first, dtype=dtype, arpb=kw.get("arpb", 0),
                           abstride=kw.get("abstride", 0))
            return gemm(a_hi, a_lo if a2 else None, pack_hi_only(wp), dtype=dtype, passes=6 if a2 else 1, bias=tab, seg_rows=seg_rows, **kw)
        # no table: 6 -> 3 (every preset with passes == 6 packs the `lo` planes three passes need), 5 -> 4 (-> 2 inside mer_gemm16)
        assert wp.lo is not None, "passes 5 / 6 need the `lo` weight plane (mer_tf_config.passes)"
        passes = 3 if a2 else 4
    return gemm(a_hi, a_lo, wp, dtype=dtype, passes=passes, bias=bias, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# one transformer block
# ------------------------------------------------------------------------------------------------------------------------------
class Layer:
    """The operands of one block, packed from host fp32 tensors: w = dict(wq, bq, wk, bk, wv, bv, wo, bo, ln1, w1, b1, w2, b2, ln2
    [, attn_bias [H, T, ceil4 T], gru_w, gru_b, gru_const]); a missing q / k / v bias is zeros."""

    def __init__(self, c, w, dev, mis=()):
        D = c.D
        z = torch.zeros(D)
        f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous().to(dev)   # noqa: E731
        kw = dict(dtype=c.dtype, passes=c.passes, dev=dev)
        self.c, self.dev, self.mis = c, dev, tuple(mis)
        wq, wk, wv = w["wq"], w["wk"], w["wv"]
        self.bqkv = f(torch.cat([w["bq"] if w.get("bq") is not None else z, w["bk"] if w.get("bk") is not None else z,
                                 w["bv"] if w.get("bv") is not None else z]))
        self.wqkv = pack(torch.cat([wq, wk, wv], 0), **kw)
        # the sub-ranges of the fused weight, each packed on its own (un-offset pointers)
        self.wqk = pack(torch.cat([wq, wk], 0), dtype=c.dtype, passes=1, dev=dev)
        self.wv = pack(wq if "v_from_q" in mis else wv, **kw)
        if "v_from_q" in mis:     # V's GEMM keeps V's hi plane; only its correction planes come from the Q rows
            good = pack(wv, **kw)
            self.wv.hi, self.wv.hb, self.wv.hp, self.wv.hq = good.hi, good.hb, good.hp, good.hq
        # the plane the fused QKV table is built from (n_first = 2 D: only the V rows of it are read for corrected columns)
        self.qkv_table_lo = pack(torch.cat([wq, wk, wq], 0), **kw).lo if ("v_from_q" in mis and c.passes >= 2) else None
        self.wkv = pack(torch.cat([wk, wv], 0), mx=(D % 256 == 0 or "kv_mx" in mis), **kw)    # CLS-only block: MX / blocked planes only when D % 256 == 0
        self.wq = pack(wq, mx=False, blk=False, **kw)                     # ... its Q GEMM reads the row-major planes alone
        self.wo, self.bo = pack(w["wo"], **kw), f(w["bo"])
        self.w1, self.b1 = pack(w["w1"], **kw), f(w["b1"])
        self.w2, self.b2 = pack(w["w2"], **kw), f(w["b2"])
        self.ln1, self.ln2 = (f(w["ln1"][0]), f(w["ln1"][1])), (f(w["ln2"][0]), f(w["ln2"][1]))
        self.attn_bias = f(w.get("attn_bias"))
        self.gru = (f(w["gru_w"]), f(w["gru_b"]), f(w["gru_const"].reshape(-1))) if w.get("gru_w") is not None else None


def _e(shape, dt, dev):
    return torch.empty(shape, dtype=dt, device=dev)


def block(x, Lw, Bseq, T, *, kv_len=None, pos_bias=None):
    """One transformer block on its fp32 input state x [Bseq*T, D] -> the next state [Bseq*T, D] (a new tensor).
    Post-LN: x is the normalised state and its 16-bit planes are split16(x); pre-LN: x is the raw residual stream."""
    _lib, ops = _ops()
    c, dev, mis = Lw.c, Lw.dev, Lw.mis
    D, F, H, ps, dt = c.D, c.F, c.H, c.passes, c.dtype
    M = Bseq * T
    t16 = ops.torch16(dt)
    lo = ps in (3, 6)
    sel = ps in (4, 5)
    ps1 = 1 if (sel and c.mx_skip & 2) else ps
    ps2 = 1 if (sel and c.mx_skip & 4) else ps
    scale = 1.0 / (D // H) ** 0.5
    assert x.shape == (M, D) and x.is_contiguous()
    tr = Lw.trace = dict(cls_only=False, tiles=None, corr={})
    ck = dict(dtype=dt, seg_rows=T, valid=kv_len, mis=mis, trace=tr["corr"])
    gin32 = None
    if c.pre_ln:
        gin32, cur_hi, cur_lo = ops.layernorm(x, Lw.ln1[0], Lw.ln1[1], c.eps, out32=c.gated, out16=True, out16_lo=lo, dtype=dt)
    else:
        cur_hi, cur_lo = ops.split16(x, dt, lo=lo)
    ab = Lw.attn_bias if Lw.attn_bias is not None else pos_bias
    f32attn = (ps == 3 or (ps == 6 and c.attn_f32)) and ab is None
    # mx_skip bit 0 under passes 5 / 6: the Q | K columns take the plain bias (n_first must be a multiple of 16: hidden = 64 * heads is)
    n_first = 2 * D if ((c.mx_skip & 1) and "n_first0" not in mis) else 0
    qkv16 = _e((M, 3 * D), t16, dev)
    qkv32 = None
    if ps == 4 and (c.mx_skip & 1) and (2 * D) % 256 == 0 and Lw.wqkv.mx is not None:
        tr["qkv"] = "split: qk one pass + v"
        corrected_gemm(cur_hi, None, Lw.wqk, Lw.bqkv[:2 * D], dtype=dt, passes=1, c16=qkv16[:, :2 * D], name="qk", trace=tr["corr"])
        corrected_gemm(cur_hi, cur_lo, Lw.wv, Lw.bqkv[2 * D:], passes=ps, c16=qkv16[:, 2 * D:], name="v", **ck)
    elif f32attn:
        tr["qkv"] = "fused fp32"
        qkv32 = _e((M, 3 * D), torch.float32, dev)
        corrected_gemm(cur_hi, cur_lo, Lw.wqkv, Lw.bqkv, passes=ps, n_first=n_first, c32=qkv32, table_lo=Lw.qkv_table_lo, name="qkv", **ck)
    else:
        tr["qkv"] = "fused"
        corrected_gemm(cur_hi, cur_lo, Lw.wqkv, Lw.bqkv, passes=ps, n_first=n_first, c16=qkv16, table_lo=Lw.qkv_table_lo, name="qkv", **ck)
    ctx_hi = _e((M, D), t16, dev)
    ctx_lo = _e((M, D), t16, dev) if lo else None
    tr["attention"] = "f32" if f32attn else ("plain" if ab is None else ("bias+gate" if Lw.gru is not None else "bias"))
    tr["ffn"] = "swiglu" if c.swiglu else "plain"
    if f32attn:
        ops.attention_f32(qkv32, Bseq, T, H, scale, kv_len=kv_len, dtype=dt, out=(ctx_hi, ctx_lo))
    elif ab is not None:
        gate = None
        if Lw.gru is not None:
            gate = ops.wavlm_gate(gin32 if c.pre_ln else x, Lw.gru[0], Lw.gru[1], Lw.gru[2], Bseq, T, H)
        assert ab.shape[2] == (T + 3) // 4 * 4
        # (the score-bias kernel writes the hi plane; the library hands it a lo plane too under two-plane presets)
        _lib.check(_lib.lib().mer_attention_bias(qkv16.data_ptr(), qkv16.data_ptr() + D * 2, qkv16.data_ptr() + 4 * D, 3 * D, ctx_hi.data_ptr(),
                                                 _ptr(ctx_lo), D, Bseq, T, H, float(scale), _ptr(kv_len), ab.data_ptr(), ab.shape[2], _ptr(gate),
                                                 ops.dt_code(dt), ops.stream()), "mer_attention_bias")
    else:
        ops.attention(qkv16, Bseq, T, H, scale, kv_len=kv_len, out=(ctx_hi, ctx_lo))
    t32 = _e((M, D), torch.float32, dev)
    corrected_gemm(ctx_hi, ctx_lo, Lw.wo, Lw.bo, passes=ps, residual=x, c32=t32, name="wo", **ck)
    f_hi = _e((M, F), t16, dev)
    f_lo = _e((M, F), t16, dev) if lo else None
    y = _e((M, D), torch.float32, dev)
    if c.pre_ln:
        _, h_hi, h_lo = ops.layernorm(t32, Lw.ln2[0], Lw.ln2[1], c.eps, out32=False, out16=True, out16_lo=lo, dtype=dt)
        if c.swiglu:
            ffn32 = _e((M, 2 * F), torch.float32, dev)
            corrected_gemm(h_hi, h_lo, Lw.w1, Lw.b1, passes=ps1, c32=ffn32, name="fc1", **ck)
            _lib.check(_lib.lib().mer_swiglu(ffn32.data_ptr(), 2 * F, M, F, f_hi.data_ptr(), _ptr(f_lo), ops.dt_code(dt), ops.stream()), "mer_swiglu")
        else:
            corrected_gemm(h_hi, h_lo, Lw.w1, Lw.b1, passes=ps1, act=c.act, c16=f_hi, c16_lo=f_lo, name="fc1", **ck)
        corrected_gemm(f_hi, f_lo, Lw.w2, Lw.b2, passes=ps2, residual=t32, c32=y, name="fc2", **ck)
        return y
    h32, h_hi, h_lo = ops.layernorm(t32, Lw.ln1[0], Lw.ln1[1], c.eps, out32=True, out16=True, out16_lo=lo, dtype=dt)
    corrected_gemm(h_hi, h_lo, Lw.w1, Lw.b1, passes=ps1, act=c.act, c16=f_hi, c16_lo=f_lo, name="fc1", **ck)
    t2 = _e((M, D), torch.float32, dev)
    corrected_gemm(f_hi, f_lo, Lw.w2, Lw.b2, passes=ps2, residual=h32, c32=t2, name="fc2", **ck)
    ops.layernorm(t2, Lw.ln2[0], Lw.ln2[1], c.eps, out=(y, None, None), dtype=dt)
    return y


def cls_block(x, Lw, Bseq, T):
    """The CLS-only last block of a CLIP tower: x fp32 [Bseq*T, D] (raw residual stream) -> the CLS rows after the block, fp32
    [Bseq, D].  K | V for every token; Q, attention, output projection (residual = row b*T of x), LayerNorm and the FFN for the
    Bseq CLS rows alone, each its own one-row sequence for the correction table (seg_rows = 1, no valid_rows)."""
    _lib, ops = _ops()
    c, dev, mis = Lw.c, Lw.dev, Lw.mis
    D, F, H, ps, dt = c.D, c.F, c.H, c.passes, c.dtype
    M = Bseq * T
    t16 = ops.torch16(dt)
    lo = ps in (3, 6)
    sel = ps in (4, 5)
    ps1 = 1 if (sel and c.mx_skip & 2) else ps
    ps2 = 1 if (sel and c.mx_skip & 4) else ps
    scale = 1.0 / (D // H) ** 0.5
    _, cur_hi, cur_lo = ops.layernorm(x, Lw.ln1[0], Lw.ln1[1], c.eps, out32=False, out16=True, out16_lo=lo, dtype=dt)
    qkv16 = torch.zeros((M, 3 * D), dtype=t16, device=dev)      # (the Q columns are never read)
    n_first = D if ((c.mx_skip & 1) and "n_first0" not in mis) else 0
    tr = Lw.trace = dict(cls_only=True, tiles=D % 256 == 0, qkv="cls: kv + q", attention="cls", ffn="plain", corr={})
    corrected_gemm(cur_hi, cur_lo, Lw.wkv, Lw.bqkv[D:], dtype=dt, passes=ps, seg_rows=T, n_first=n_first, mis=mis, c16=qkv16[:, D:],
                   name="kv", trace=tr["corr"])
    one = dict(dtype=dt, seg_rows=1, mis=mis, trace=tr["corr"])
    q16 = _e((Bseq, D), t16, dev)
    rows = lambda t: None if t is None else t.view(Bseq, T * D)[:, :D]     # noqa: E731   row b = token 0 of sequence b (stride T * D)
    corrected_gemm(rows(cur_hi), rows(cur_lo), Lw.wq, Lw.bqkv[:D], passes=ps, c16=q16, name="q", **one)
    ctx_hi, ctx_lo = _e((Bseq, D), t16, dev), (_e((Bseq, D), t16, dev) if lo else None)
    ops.attention_cls(q16, qkv16, Bseq, T, H, scale, out=(ctx_hi, ctx_lo))
    t32 = _e((Bseq, D), torch.float32, dev)
    corrected_gemm(ctx_hi, ctx_lo, Lw.wo, Lw.bo, passes=ps, residual=rows(x), c32=t32, name="wo", **one)
    _, h_hi, h_lo = ops.layernorm(t32, Lw.ln2[0], Lw.ln2[1], c.eps, out32=False, out16=True, out16_lo=lo, dtype=dt)
    f_hi, f_lo = _e((Bseq, F), t16, dev), (_e((Bseq, F), t16, dev) if lo else None)
    corrected_gemm(h_hi, h_lo, Lw.w1, Lw.b1, passes=ps1, act=c.act, c16=f_hi, c16_lo=f_lo, name="fc1", **one)
    y = _e((Bseq, D), torch.float32, dev)
    corrected_gemm(f_hi, f_lo, Lw.w2, Lw.b2, passes=ps2, residual=t32, c32=y, name="fc2", **one)
    return y


def last4(hs, seg_start=None, seg_len=None):
    """frames = sum of the last four states (as many as exist), pooled = per-segment mean of frames."""
    _lib, ops = _ops()
    return ops.sum_pool(list(hs[-4:]), seg_start, seg_len, frames=True)


# ------------------------------------------------------------------------------------------------------------------------------
# state dict -> per-layer host tensors (HF key names, as documented in mertools_amd/synthetic.py)
# ------------------------------------------------------------------------------------------------------------------------------
def bert_layers(sd, n):
    out = []
    for l in range(n):
        q = f"encoder.layer.{l}."
        a = q + "attention.self."
        out.append(dict(wq=sd[a + "query.weight"], bq=sd[a + "query.bias"], wk=sd[a + "key.weight"], bk=sd[a + "key.bias"],
                        wv=sd[a + "value.weight"], bv=sd[a + "value.bias"], wo=sd[q + "attention.output.dense.weight"],
                        bo=sd[q + "attention.output.dense.bias"],
                        ln1=(sd[q + "attention.output.LayerNorm.weight"], sd[q + "attention.output.LayerNorm.bias"]),
                        w1=sd[q + "intermediate.dense.weight"], b1=sd[q + "intermediate.dense.bias"], w2=sd[q + "output.dense.weight"],
                        b2=sd[q + "output.dense.bias"], ln2=(sd[q + "output.LayerNorm.weight"], sd[q + "output.LayerNorm.bias"])))
    return out


def hubert_layers(sd, n):
    out = []
    for l in range(n):
        q = f"encoder.layers.{l}."
        a = q + "attention."
        d = dict(wq=sd[a + "q_proj.weight"], bq=sd[a + "q_proj.bias"], wk=sd[a + "k_proj.weight"], bk=sd[a + "k_proj.bias"],
                 wv=sd[a + "v_proj.weight"], bv=sd[a + "v_proj.bias"], wo=sd[a + "out_proj.weight"], bo=sd[a + "out_proj.bias"],
                 ln1=(sd[q + "layer_norm.weight"], sd[q + "layer_norm.bias"]), w1=sd[q + "feed_forward.intermediate_dense.weight"],
                 b1=sd[q + "feed_forward.intermediate_dense.bias"], w2=sd[q + "feed_forward.output_dense.weight"],
                 b2=sd[q + "feed_forward.output_dense.bias"], ln2=(sd[q + "final_layer_norm.weight"], sd[q + "final_layer_norm.bias"]))
        if a + "gru_rel_pos_linear.weight" in sd:
            d.update(gru_w=sd[a + "gru_rel_pos_linear.weight"], gru_b=sd[a + "gru_rel_pos_linear.bias"], gru_const=sd[a + "gru_rel_pos_const"])
        out.append(d)
    return out


def clip_layers(sd, n):
    out = []
    for l in range(n):
        q = f"vision_model.encoder.layers.{l}."
        a = q + "self_attn."
        out.append(dict(wq=sd[a + "q_proj.weight"], bq=sd[a + "q_proj.bias"], wk=sd[a + "k_proj.weight"], bk=sd[a + "k_proj.bias"],
                        wv=sd[a + "v_proj.weight"], bv=sd[a + "v_proj.bias"], wo=sd[a + "out_proj.weight"], bo=sd[a + "out_proj.bias"],
                        ln1=(sd[q + "layer_norm1.weight"], sd[q + "layer_norm1.bias"]), w1=sd[q + "mlp.fc1.weight"], b1=sd[q + "mlp.fc1.bias"],
                        w2=sd[q + "mlp.fc2.weight"], b2=sd[q + "mlp.fc2.bias"], ln2=(sd[q + "layer_norm2.weight"], sd[q + "layer_norm2.bias"])))
    return out


def vit_family_layers(sd, n, kind, *, window=None):
    """kind: "videomae" | "dinov2" (layer scale folded into wo / w2 and their biases) | "d2v" (no key bias, lambda_1 / lambda_2 folded,
    the relative position bias baked per layer as [H, T, ceil4(T)])."""
    from oracle import encoders_ref as R
    out = []
    shared = sd.get("encoder.relative_position_bias.relative_position_bias_table") if kind == "d2v" else None
    shared = R.beit_relative_position_bias(shared, window) if shared is not None else None
    for l in range(n):
        q = f"encoder.layer.{l}."
        a = q + "attention.attention."
        D = sd[a + "query.weight"].shape[0]
        one = torch.ones(D)
        if kind == "dinov2":
            l1, l2 = sd[q + "layer_scale1.lambda1"], sd[q + "layer_scale2.lambda1"]
            n1, n2 = "norm1", "norm2"
            sw = q + "mlp.weights_in.weight" in sd
            k1, k2 = ("mlp.weights_in", "mlp.weights_out") if sw else ("mlp.fc1", "mlp.fc2")
        else:
            l1, l2 = (sd.get(q + "lambda_1", one), sd.get(q + "lambda_2", one)) if kind == "d2v" else (one, one)
            n1, n2 = "layernorm_before", "layernorm_after"
            k1, k2 = "intermediate.dense", "output.dense"
        d = dict(wq=sd[a + "query.weight"], bq=sd[a + "query.bias"], wk=sd[a + "key.weight"], bk=sd.get(a + "key.bias"),
                 wv=sd[a + "value.weight"], bv=sd[a + "value.bias"], wo=sd[q + "attention.output.dense.weight"] * l1[:, None],
                 bo=sd[q + "attention.output.dense.bias"] * l1, ln1=(sd[q + n1 + ".weight"], sd[q + n1 + ".bias"]),
                 w1=sd[q + k1 + ".weight"], b1=sd[q + k1 + ".bias"], w2=sd[q + k2 + ".weight"] * l2[:, None], b2=sd[q + k2 + ".bias"] * l2,
                 ln2=(sd[q + n2 + ".weight"], sd[q + n2 + ".bias"]))
        if kind == "d2v":
            own = sd.get(a + "relative_position_bias.relative_position_bias_table")
            bias = R.beit_relative_position_bias(own, window) if own is not None else None
            if shared is not None:
                bias = shared if bias is None else bias + shared
            if bias is not None:
                Hn, T = bias.shape[0], bias.shape[1]
                padded = torch.zeros(Hn, T, (T + 3) // 4 * 4)
                padded[:, :, :T] = bias
                d["attn_bias"] = padded
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# whole forwards
# ------------------------------------------------------------------------------------------------------------------------------
def bert_front(sd, cfg, c, ids, dev, token_type=None):
    """hidden_states[0]: mer_bert_embed (+ the emb_dim projection, a GEMM with the block pass code and no sequence structure)."""
    _lib, ops = _ops()
    f = lambda k: sd[k].to(torch.float32).contiguous().to(dev)   # noqa: E731
    lo = c.passes in (3, 6)
    pos_mode = 1 if cfg.model_type in ("roberta", "xlm-roberta") else 0
    pad = cfg.pad_token_id if cfg.pad_token_id is not None else 0
    r = ops.bert_embed(ids, token_type, f("embeddings.word_embeddings.weight"), f("embeddings.position_embeddings.weight"),
                       f("embeddings.token_type_embeddings.weight"), pos_mode, pad, f("embeddings.LayerNorm.weight"),
                       f("embeddings.LayerNorm.bias"), cfg.layer_norm_eps, dtype=c.dtype, out16_lo=True)
    proj = "encoder.embedding_hidden_mapping_in." if "encoder.embedding_hidden_mapping_in.weight" in sd else "embeddings_project."
    if proj + "weight" not in sd:
        return r[0]
    wp = pack(sd[proj + "weight"], dtype=c.dtype, passes=c.passes, dev=dev)
    h0 = _e((ids.numel(), c.D), torch.float32, dev)
    h16 = _e((ids.numel(), c.D), ops.torch16(c.dtype), dev)
    corrected_gemm(r[1], r[2] if lo else None, wp, f(proj + "bias"), dtype=c.dtype, passes=c.passes, c32=h0, c16=h16,
                   c16_lo=torch.empty_like(h16) if lo else None)
    return h0


def vit_front(patch_w, patch_b, cls, pos, pre_ln, c, px, P, dev, mis=()):
    """mer_vit_patchify + the patch GEMM (one sequence = the P*P patch rows of an image) + mer_vit_assemble -> x fp32 [N*(1+np), D]."""
    _lib, ops = _ops()
    f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous().to(dev)   # noqa: E731
    lo = c.passes in (3, 6)
    N = px.shape[0]
    npatch = (px.shape[2] // P) ** 2
    p_hi, p_lo = ops.vit_patchify(px, P, dtype=c.dtype, lo=lo)
    pw = patch_w.reshape(c.D, -1)
    padc = (-pw.shape[1]) % 8
    if padc:
        pw = torch.cat([pw, torch.zeros(pw.shape[0], padc)], 1)
    wp = pack(pw, dtype=c.dtype, passes=c.passes, dev=dev)
    patch32 = _e((N * npatch, c.D), torch.float32, dev)
    corrected_gemm(p_hi, p_lo, wp, f(patch_b), dtype=c.dtype, passes=c.passes, seg_rows=npatch, mis=mis, c32=patch32)
    g, b = (f(pre_ln[0]), f(pre_ln[1])) if pre_ln is not None else (None, None)
    return ops.vit_assemble(patch32, f(cls.reshape(-1)), f(pos), g, b, c.eps, N, npatch, c.D, dtype=c.dtype)


def clip_forward(sd, cfg, c, px, dev, *, cls_path, mis=(), traces=None):
    """CLIP image_features [N, proj_dim]; cls_path: the last block is the CLS-only block (what mer_vit_forward runs when no token
    states are asked for) or a full block (mer_vit_forward_tokens with tokens_out).  -> (features, last residual stream or None)."""
    _lib, ops = _ops()
    vc = cfg.vision_config
    v = "vision_model."
    N = px.shape[0]
    T = (vc.image_size // vc.patch_size) ** 2 + 1
    x = vit_front(sd[v + "embeddings.patch_embedding.weight"], None, sd[v + "embeddings.class_embedding"],
                  sd[v + "embeddings.position_embedding.weight"], (sd[v + "pre_layrnorm.weight"], sd[v + "pre_layrnorm.bias"]), c, px,
                  vc.patch_size, dev, mis)
    layers = clip_layers(sd, c.layers)
    for l in range(c.layers):
        Lw = Layer(c, layers[l], dev, mis)
        if cls_path and l == c.layers - 1:
            rows = cls_block(x, Lw, N, T)
            x = None
        else:
            x = block(x, Lw, N, T)
        if traces is not None:
            traces.append(Lw.trace)      # the path each block took, for the comparison with expected_path
    if x is not None:
        rows = x.view(N, T * c.D)[:, :c.D]
    lo = c.passes in (3, 6)
    f = lambda k: sd[k].to(torch.float32).contiguous().to(dev)   # noqa: E731
    _, h_hi, h_lo = ops.layernorm(rows, f(v + "post_layernorm.weight"), f(v + "post_layernorm.bias"), c.eps, out32=False, out16=True,
                                  out16_lo=lo, dtype=c.dtype, M=N, D=c.D, ldx=rows.stride(0))
    wp = pack(sd["visual_projection.weight"], dtype=c.dtype, passes=c.passes, dev=dev)
    feats = _e((N, cfg.projection_dim), torch.float32, dev)
    corrected_gemm(h_hi, h_lo, wp, None, dtype=c.dtype, passes=c.passes, c32=feats)      # no sequence structure: 5 -> 4 -> 2, 6 -> 3
    return feats, x


def tokensum_forward(sd, cfg, c, px, dev, kind, pos, traces=None):
    """DINOv2 / data2vec-vision: patch GEMM with bias, no embedding LayerNorm, full blocks, features = token sum of the last
    residual stream.  -> (features [N, D], tokens [N, T, D])."""
    _lib, ops = _ops()
    P = cfg.patch_size
    N = px.shape[0]
    win = px.shape[2] // P
    T = win * win + 1
    x = vit_front(sd["embeddings.patch_embeddings.projection.weight"], sd["embeddings.patch_embeddings.projection.bias"],
                  sd["embeddings.cls_token"], pos, None, c, px, P, dev)
    layers = vit_family_layers(sd, c.layers, kind, window=win)
    for l in range(c.layers):
        Lw = Layer(c, layers[l], dev)
        x = block(x, Lw, N, T)
        if traces is not None:
            traces.append(Lw.trace)
    return ops.token_reduce(x.view(N, T, c.D)), x.view(N, T, c.D)


def videomae_forward(sd, cfg, c, px, dev, seg_start=None, seg_len=None, traces=None):
    """-> (last_hidden_state [B*NP, D], pooled or None)."""
    from oracle import encoders_ref as R
    _lib, ops = _ops()
    f = lambda t: t.detach().to(torch.float32).contiguous().to(dev)   # noqa: E731
    lo = c.passes in (3, 6)
    B = px.shape[0]
    NP = (cfg.image_size // cfg.patch_size) ** 2 * (cfg.num_frames // cfg.tubelet_size)
    p_hi, p_lo = ops.video_patchify(px, cfg.patch_size, cfg.tubelet_size, dtype=c.dtype, lo=lo)
    wp = pack(sd["embeddings.patch_embeddings.projection.weight"].reshape(c.D, -1), dtype=c.dtype, passes=c.passes, dev=dev)
    x = _e((B * NP, c.D), torch.float32, dev)
    corrected_gemm(p_hi, p_lo, wp, f(sd["embeddings.patch_embeddings.projection.bias"]), dtype=c.dtype, passes=c.passes, seg_rows=NP, c32=x)
    ops.add_pos(x, f(R.videomae_sinusoid(NP, c.D)))
    layers = vit_family_layers(sd, c.layers, "videomae")
    for l in range(c.layers):
        Lw = Layer(c, layers[l], dev)
        x = block(x, Lw, B, NP)
        if traces is not None:
            traces.append(Lw.trace)
    if "layernorm.weight" in sd:
        ops.layernorm(x, f(sd["layernorm.weight"]), f(sd["layernorm.bias"]), c.eps, out=(x, None, None), dtype=c.dtype)
    pooled = ops.sum_pool([x], seg_start, seg_len)[1] if seg_start is not None else None
    return x, pooled


def hubert_front(sd, cfg, c, wav, dev, valid_samples=None):
    """conv0 (GroupNorm or LayerNorm front end) -> implicit-im2col conv GEMMs -> feature projection -> positional conv (+ the
    encoder LayerNorm of the post-LN encoder) -> (hidden_states[0] fp32 [B*T, D], T, tn_len or None)."""
    from oracle import encoders_ref as R
    _lib, ops = _ops()
    f = lambda t: None if t is None else t.detach().to(torch.float32).contiguous().to(dev)   # noqa: E731
    dt, cps, tps = c.dtype, c.conv_passes, c.passes
    t16 = ops.torch16(dt)
    B, L = wav.shape
    Cc, D = cfg.conv_dim[0], c.D
    ks, ss = list(cfg.conv_kernel), list(cfg.conv_stride)
    n = len(ks)
    group = cfg.feat_extract_norm == "group"
    fp_ln = bool(getattr(cfg, "feat_proj_layer_norm", True))
    stable = bool(getattr(cfg, "do_stable_layer_norm", False))
    clo = cps == 3
    Ts, t = [], L
    for i in range(n):
        t = (t - ks[i]) // ss[i] + 1
        Ts.append(t)
    Tn = Ts[-1]
    M = B * Tn
    vlen = ops.hubert_valid_frames(valid_samples, L, ks, ss, all_layers=True) if valid_samples is not None else None
    t0_len = vlen[0] if vlen is not None else None
    tn_len = vlen[n - 1] if vlen is not None else None
    fe = "feature_extractor.conv_layers."
    ng = lambda i: (f(sd.get(fe + f"{i}.layer_norm.weight")), f(sd.get(fe + f"{i}.layer_norm.bias")))   # noqa: E731
    cb = lambda i: f(sd[fe + f"{i}.conv.bias"]) if cfg.conv_bias else None   # noqa: E731
    w0 = f(sd[fe + "0.conv.weight"].reshape(Cc, -1))
    if group:
        src = ops.hubert_conv0_gn(wav, w0, ng(0)[0], ng(0)[1], 1e-5, stride=ss[0], dtype=dt, lo=clo, valid_frames=t0_len)
    else:
        c32 = ops.hubert_conv0_plain(wav, w0, cb(0), stride=ss[0])
        _, h, l_ = ops.layernorm(c32, ng(0)[0], ng(0)[1], 1e-5, act="gelu", out32=False, out16=True, out16_lo=clo, dtype=dt)
        src = (h, l_)
    last32 = fp16 = None
    for i in range(1, n):
        last = i == n - 1
        wp = pack(sd[fe + f"{i}.conv.weight"].permute(0, 2, 1).reshape(Cc, -1), dtype=dt, passes=cps, dev=dev)
        Mi = B * Ts[i]
        kw = dict(dtype=dt, passes=cps, M=Mi, lda=ss[i] * Cc, arpb=Ts[i], abstride=Ts[i - 1] * Cc,
                  seg_rows=Ts[i] if cps == 5 else 0, valid=vlen[i] if vlen is not None else None)
        a_hi, a_lo = src[0].view(-1, Cc), (src[1].view(-1, Cc) if src[1] is not None else None)
        o_hi, o_lo = _e((Mi, Cc), t16, dev), (_e((Mi, Cc), t16, dev) if clo else None)
        if group:
            want16 = (not last) or (not fp_ln)
            last32 = _e((Mi, Cc), torch.float32, dev) if last else None
            corrected_gemm(a_hi, a_lo, wp, cb(i), act="gelu", c32=last32, c16=o_hi if want16 else None, c16_lo=o_lo if want16 else None, **kw)
        else:
            c32 = _e((Mi, Cc), torch.float32, dev)
            corrected_gemm(a_hi, a_lo, wp, cb(i), c32=c32, **kw)
            # the last conv's LayerNorm feeds the projection's LayerNorm in fp32 when there is one, else the projection in 16 bits
            last32 = _e((Mi, Cc), torch.float32, dev) if (last and fp_ln) else None
            ops.layernorm(c32, ng(i)[0], ng(i)[1], 1e-5, act="gelu", out=(last32,) + ((None, None) if last32 is not None else (o_hi, o_lo)),
                          dtype=dt)
        src = (o_hi, o_lo)
    fp16 = src
    if fp_ln:
        _, h, l_ = ops.layernorm(last32, f(sd["feature_projection.layer_norm.weight"]), f(sd["feature_projection.layer_norm.bias"]), c.eps,
                                 out32=False, out16=True, out16_lo=clo, dtype=dt)
        fp16 = (h, l_)
    # feature projection (mer_hubert_config.conv_passes): the per-sequence table under conv_passes == 5, and behind the projection's
    # LayerNorm under tf.passes 5 / 6 too; on two MFMA passes where the conv stack hands over hi + lo planes (conv_passes == 3)
    proj_table = cps == 5 or (tps in (5, 6) and fp_ln)
    proj_passes = (6 if clo else 5) if proj_table else cps
    wfp = pack(sd["feature_projection.projection.weight"], dtype=dt, passes=cps, dev=dev)
    hproj = _e((M, D), torch.float32, dev)
    corrected_gemm(fp16[0], fp16[1], wfp, f(sd["feature_projection.projection.bias"]), dtype=dt, passes=proj_passes,
                   seg_rows=Tn if proj_table else 0, valid=tn_len, c32=hproj)
    # positional conv: x + GELU(grouped conv(x)) as ONE batched GEMM over (clip, group); conv_passes 4 / 5 run it as 2 (mer_hubert_config.conv_passes)
    G, K = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings
    Dg = D // G
    pw = R.pos_conv_weight(sd).reshape(G, Dg, Dg, K).permute(0, 1, 3, 2).reshape(G * Dg, K * Dg)
    wpos = pack(pw, dtype=dt, passes=2 if cps >= 2 else 1, dev=dev, blk=False)
    pk_hi, pk_lo = ops.posconv_pack(hproj.view(B, Tn, D), G, K, dtype=dt, lo=clo, valid_frames=tn_len)
    out0 = _e((M, D), torch.float32, dev)
    g = _lib.GemmArgs()
    g.M, g.N, g.K, g.dtype = Tn, Dg, K * Dg, ops.dt_code(dt)
    g.a_hi, g.a_lo, g.lda = pk_hi.data_ptr(), _ptr(pk_lo), Dg
    g.w_hi, g.w_lo, g.ldw = wpos.hi.data_ptr(), _ptr(wpos.lo), K * Dg
    bias_t = f(sd["encoder.pos_conv_embed.conv.bias"])
    g.bias = bias_t.data_ptr()
    g.nbatch, g.nb_inner = B * G, G
    g.a_so, g.a_si = G * (Tn + K) * Dg, (Tn + K) * Dg
    g.w_si, g.bias_si = Dg * K * Dg, Dg
    g.c_so, g.c_si = Tn * D, Dg
    g.passes = 2 if cps in (4, 5) else cps
    g.act = ops.ACT["gelu"]
    g.residual, g.ldr = hproj.data_ptr(), D
    g.c32, g.ldc32 = out0.data_ptr(), D
    ops.gemm16_raw(g)
    if not stable:
        out0 = ops.layernorm(out0, f(sd["encoder.layer_norm.weight"]), f(sd["encoder.layer_norm.bias"]), c.eps, dtype=dt)[0]
    return out0, Tn, tn_len


def wavlm_bias(sd, cfg, T, dev):
    """The [H, T, ceil4(T)] relative position bias table of a WavLM checkpoint (None for HuBERT / wav2vec2)."""
    from oracle import encoders_ref as R
    k = "encoder.layers.0.attention.rel_attn_embed.weight"
    if k not in sd:
        return None
    tab = R.wavlm_position_bias(sd[k], T, getattr(cfg, "num_buckets", 320), getattr(cfg, "max_bucket_distance", 800))
    padded = torch.zeros(tab.shape[0], T, (T + 3) // 4 * 4)
    padded[:, :, :T] = tab
    return padded.contiguous().to(dev)


def hubert_final_ln(sd, c, h, dev):
    """The stable-LN encoder's final LayerNorm, applied to the last state only (in place in the library; a new tensor here)."""
    _lib, ops = _ops()
    f = lambda t: t.detach().to(torch.float32).contiguous().to(dev)   # noqa: E731
    return ops.layernorm(h.contiguous(), f(sd["encoder.layer_norm.weight"]), f(sd["encoder.layer_norm.bias"]), c.eps, dtype=c.dtype)[0]


# ------------------------------------------------------------------------------------------------------------------------------
# the case table (pure data: the GPU tests run it, the CPU test asserts what it reaches)
# ------------------------------------------------------------------------------------------------------------------------------
BIG, SMALL = (16, 64), (3, 24)      # (B, T): 1024 rows of 64-token sequences (256x256 tiles, persistent kernel, staged table) | ragged, T < 40


def _b(D, F, preset, skip, dtype="f16", rows=SMALL, layers=2, emb=None):
    return dict(D=D, F=F, preset=preset, skip=skip, dtype=dtype, rows=rows, layers=layers, emb=emb)


BERT_CASES = [
    _b(128, 256, "fast", 1), _b(128, 256, "mean", 1, layers=7), _b(128, 320, "mx", 1, rows=BIG), _b(128, 256, "accurate", 0),
    _b(128, 256, "mean", 7, rows=BIG, emb=64), _b(128, 256, "x3_conv4", 1, "bf16"),
    _b(192, 256, "mx", 1, rows=BIG), _b(192, 320, "mean", 1), _b(192, 256, "mean_a2", 1, "bf16", rows=BIG), _b(192, 256, "balanced", 0),
    _b(192, 256, "mean_conv3", 7),
    _b(256, 256, "mx", 1, rows=BIG), _b(256, 320, "mx", 7), _b(256, 256, "mean", 1, rows=BIG), _b(256, 256, "mean", 7),
    _b(256, 256, "mean_a2f", 1, rows=BIG), _b(256, 256, "mx", 1, "bf16"), _b(256, 320, "a2_conv3", 0), _b(256, 256, "mean_conv3", 2),
    _b(256, 256, "mean", 4, rows=BIG), _b(256, 256, "mx", 0, rows=BIG, emb=64), _b(256, 256, "fast", 1, rows=BIG),
    _b(384, 256, "mx", 1, rows=BIG), _b(384, 320, "mx", 0), _b(384, 256, "mean", 1), _b(384, 256, "mean", 7, "bf16", rows=BIG),
    _b(384, 256, "accurate", 1), _b(384, 256, "mean_a2", 0, rows=BIG), _b(384, 256, "balanced", 1, rows=BIG), _b(384, 320, "mean_all", 1),
    _b(384, 256, "mean_conv", 7),
]


def _h(D, F, preset, skip, *, norm="group", stable=False, wavlm=False, L=4000, B=2, ragged=False, dtype="f16"):
    return dict(D=D, F=F, preset=preset, skip=skip, norm=norm, stable=stable, wavlm=wavlm, L=L, B=B, ragged=ragged, dtype=dtype, layers=2)


HUBERT_CASES = [
    _h(128, 256, "mean", 1, L=8000, B=3, ragged=True), _h(128, 256, "x3_conv4", 1), _h(128, 256, "mean_all", 1, L=8000, B=3, ragged=True),
    _h(128, 256, "mean_conv", 7, norm="layer", stable=True), _h(128, 320, "mean_a2f", 1, wavlm=True, L=8000),
    _h(192, 256, "mean_a2", 1, wavlm=True, B=3, ragged=True), _h(192, 320, "accurate", 0, norm="layer", stable=True, L=8000),
    _h(256, 320, "mean", 7, norm="layer", stable=True, L=8000), _h(256, 256, "mx", 1, L=8000), _h(256, 256, "mean_conv3", 1, B=3, ragged=True),
    _h(256, 256, "balanced", 7, dtype="bf16"),
    _h(256, 256, "a2_conv3", 7, norm="layer", stable=True, wavlm=True, B=3, ragged=True),
    _h(384, 256, "mx", 1, L=8000), _h(384, 256, "mean", 1, wavlm=True), _h(384, 320, "fast", 0, norm="layer", stable=True),
]


def _c(D, F, preset, skip, *, dtype="f16", image=64, patch=16, N=5):
    return dict(D=D, F=F, preset=preset, skip=skip, dtype=dtype, image=image, patch=patch, N=N, layers=2)


CLIP_CASES = [
    _c(128, 256, "mean", 7), _c(128, 320, "mx", 1, image=56, patch=14), _c(128, 256, "accurate", 7),
    _c(192, 256, "mean_a2", 7), _c(192, 256, "mx", 0), _c(192, 320, "mean_a2f", 1),
    _c(256, 256, "mx", 7, N=64), _c(256, 320, "mean", 1, image=56, patch=14), _c(256, 256, "balanced", 7, dtype="bf16"),
    _c(256, 256, "mean", 7, N=64), _c(256, 256, "mx", 1), _c(256, 256, "fast", 0),
    _c(384, 256, "mx", 1), _c(384, 256, "mean", 7), _c(384, 320, "mx", 7, dtype="bf16"), _c(384, 256, "a2_conv3", 1),
    _c(192, 320, "mean", 2), _c(128, 256, "mx", 4),      # mx_skip bits 1 / 2 alone, under the pass codes that read them (4 / 5)
]
# (kind, D, preset, mx_skip): DINOv2-giant style SwiGLU, data2vec-vision with a baked attn_bias, VideoMAE with its final LayerNorm
TOKSUM_CASES = [("dinov2", 128, "mean", 7), ("dinov2", 256, "mx", 1), ("dinov2", 384, "accurate", 7),
                ("d2v", 128, "mean", 7), ("d2v", 256, "mx", 1), ("d2v", 192, "accurate", 0), ("d2v", 384, "mean_a2", 7)]
VMAE_CASES = [(128, 256, "mean", 7), (256, 320, "mx", 7), (384, 256, "mean_a2", 1), (192, 256, "balanced", 0)]
