"""BLOOM text encoder, the part that needs no GPU: the two C entry points are exported, bound and refuse bad arguments on the host;
ops.alibi_slopes IS build_alibi_tensor's slopes; HipBloomModel refuses every config it does not cover, naming the field; tests/bloom_refs.py
— the float64 formulas the GPU tests lean on — IS HF's BloomModel (eager, fp32); and the two elementwise bounds the GPU tests hold the
kernels to admit plain fp32 torch and reject the kernels they are meant to catch."""
import ctypes
import os

import pytest
import torch

import bloom_refs as R
from op_refs import worst_ratio
from util import rel_err


@pytest.fixture(scope="module")
def lib():
    from mertools_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mertools_amd import build
        build.build()
    return _lib.lib()


@pytest.fixture(scope="module", params=sorted(R.TINY))
def tiny(request):
    return request.param, R.tiny_bloom(request.param)


def test_entry_points_are_exported_and_bound(lib):
    from mertools_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mer_hip.h")).read()
    for name in ("mer_layernorm_row", "mer_alibi_attention"):
        assert hasattr(lib, name) and name in _lib._PROTOS, name
        assert name in header
    assert callable(ops.layernorm_row) and callable(ops.alibi_attention) and callable(ops.alibi_slopes)


def test_bad_arguments_fail_on_the_host(lib):
    """The pointers are host memory and are never dereferenced: every refusal is decided before a launch."""
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    f = ctypes.c_float
    ok_norm = dict(x=p, ldx=8, gamma=None, beta=None, eps=f(1e-5), M=1, D=8, out32=p, ld32=8, hi=None, lo=None, ld16=8, dtype=0)

    def norm(**kw):
        a = dict(ok_norm, **kw)
        return lib.mer_layernorm_row(a["x"], a["ldx"], a["gamma"], a["beta"], a["eps"], a["M"], a["D"], a["out32"], a["ld32"], a["hi"], a["lo"],
                                     a["ld16"], a["dtype"], None)
    for kw in (dict(D=6, ldx=8), dict(D=8196, ldx=8196, ld32=8196), dict(x=None), dict(M=0), dict(out32=None), dict(dtype=2), dict(ldx=4),
               dict(lo=p), dict(beta=p + 4), dict(gamma=p + 8)):
        assert norm(**kw) < 0, kw
        assert b"mer_layernorm_row" in lib.mer_last_error(), (kw, lib.mer_last_error())
    ok_att = dict(q=p, k=p, v=p, ld=384, slopes=p, hi=p, lo=None, ldo=128, B=1, T=4, H=1, hd=128, dtype=0)

    def att(**kw):
        a = dict(ok_att, **kw)
        return lib.mer_alibi_attention(a["q"], a["k"], a["v"], a["ld"], a["slopes"], a["hi"], a["lo"], a["ldo"], a["B"], a["T"], a["H"], a["hd"],
                                       f(1.0), a["dtype"], None)
    for kw in (dict(hd=72), dict(T=0), dict(T=2049), dict(slopes=None), dict(q=None), dict(k=None), dict(v=None), dict(hi=None), dict(B=0), dict(H=0),
               dict(ld=100), dict(ldo=64), dict(hd=32), dict(hd=256), dict(dtype=3), dict(q=p + 4), dict(slopes=p + 2)):
        assert att(**kw) < 0, kw
        assert b"mer_alibi_attention" in lib.mer_last_error(), (kw, lib.mer_last_error())
    # the same refusals carry the same codes as mer_rope_attention's
    for kw in (dict(hd=72), dict(T=2049), dict(B=0), dict(ld=100), dict(q=p + 4), dict(dtype=3), dict(hi=None)):
        a = dict(ok_att, **kw)
        rope = lib.mer_rope_attention(a["q"], a["k"], a["v"], a["ld"], p, p, a["hi"], a["lo"], a["ldo"], a["B"], a["T"], a["H"], a["hd"], f(1.0), a["dtype"], None)
        assert att(**kw) == rope, kw


@pytest.mark.parametrize("H", [1, 2, 3, 6, 8, 12, 32, 40])
def test_alibi_slopes_are_build_alibi_tensors(H):
    from mertools_amd import ops
    got = ops.alibi_slopes(H)
    assert got.dtype == torch.float32 and got.shape == (H,)
    assert torch.equal(got, R.hf_slopes(H)), (H, got, R.hf_slopes(H))
    if H == 3:
        assert got.tolist() == [0.0625, 0.00390625, 0.25]
    if H == 32:
        assert float(got[0]) == float(torch.tensor(R.STEEPEST, dtype=torch.float32)) == float(got.max())


def _config(**kw):
    import transformers as tr
    base = dict(hidden_size=256, n_head=2, n_layer=1, vocab_size=32)
    base.update(kw)
    return tr.BloomConfig(**base)


@pytest.mark.parametrize("field,make", [
    ("model_type", lambda: __import__("transformers").GPT2Config(n_embd=256, n_head=2, n_layer=1, vocab_size=32)),
    ("head_dim", lambda: _config(hidden_size=192, n_head=2)),          # head_dim 96
    ("head_dim", lambda: _config(hidden_size=256, n_head=8)),          # head_dim 32
    ("head_dim", lambda: _config(hidden_size=256, n_head=3)),          # 256 / 3 is no integer
    ("hidden_size", lambda: _config(hidden_size=8320, n_head=65)),     # head_dim 128, wider than mer_layernorm_row holds
    ("hidden_size", lambda: _config(hidden_size=132, n_head=2)),       # no multiple of 8
])
def test_unsupported_configs_are_refused_by_name(field, make):
    """Refused at construction, before a weight is read (the state dict is empty) and before the library or a GPU is needed."""
    from mertools_amd.bloom import HipBloomModel, check_config
    cfg = make()
    with pytest.raises(ValueError, match=field) as ei:
        HipBloomModel({}, cfg, device="cpu")
    value = {"model_type": cfg.model_type, "head_dim": cfg.hidden_size // getattr(cfg, "n_head", 1)}.get(field, getattr(cfg, field, None))
    assert str(value) in str(ei.value), ei.value
    with pytest.raises(ValueError, match=field):
        check_config(cfg)


def test_supported_configs_pass_the_check():
    from mertools_amd.bloom import check_config
    assert check_config(_config()) == (256, 2, 128, 1, False)
    assert check_config(_config(hidden_size=192, n_head=3, apply_residual_connection_post_layernorm=True)) == (192, 3, 64, 1, True)
    assert check_config(_config(hidden_size=4096, n_head=32, n_layer=30, pretraining_tp=4, slow_but_exact=True))[:4] == (4096, 32, 128, 30)
    assert check_config(_config(hidden_size=8192, n_head=64))[:3] == (8192, 64, 128)


def test_query_key_value_rows_are_permuted_into_blocks():
    """Row h * 3 * hd + c * hd + d of HF's fused projection (view [H, 3, hd]) becomes row c * D + h * hd + d."""
    from mertools_amd.bloom import _qkv_blocks
    H, hd = 3, 64
    D = H * hd
    w = torch.arange(3 * D * 2, dtype=torch.float32).reshape(3 * D, 2)
    out, outb = _qkv_blocks(w, H, hd), _qkv_blocks(w[:, 0].contiguous(), H, hd)
    for h, c, d in ((0, 0, 0), (2, 1, 5), (1, 2, 63), (2, 2, 63)):
        assert torch.equal(out[c * D + h * hd + d], w[h * 3 * hd + c * hd + d]) and outb[c * D + h * hd + d] == w[h * 3 * hd + c * hd + d, 0]
    assert sorted(out[:, 0].tolist()) == w[:, 0].tolist()


def test_float64_forward_is_the_hf_module(tiny):
    name, m = tiny
    ids = R.batch_ids(lengths=(17,))
    ref = R.hf_hidden_states(m, ids)
    got = R.bloom_forward64(m.state_dict(), m.config, ids)
    assert len(got) == len(ref) == m.config.n_layer + 1
    worst = max(rel_err(r, g)[0] for r, g in zip(ref, got))
    print(f"bloom_forward64 vs HF fp32 [{name}]: worst hidden state {worst:.2e}")
    assert worst <= 5e-6


def test_relative_and_absolute_bias_are_the_same_attention():
    """softmax's shift invariance in float64: slope * (j - t) against HF's slope * j."""
    B, T, H, hd = 2, 65, 3, 64
    D = H * hd
    x = R.attention_inputs(B, T, H, hd, seed=3)
    q, k, v = x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D]
    slopes = R.hf_slopes(H)
    rel = R.alibi_attention_ref(q, k, v, slopes, B, T, H, hd, 1.0)
    assert rel_err(R.alibi_attention_ref(q, k, v, slopes, B, T, H, hd, 1.0, relative=False), rel)[0] <= 1e-13


@pytest.mark.parametrize("steepest", [False, True], ids=["bloom", "steepest"])
@pytest.mark.parametrize("shape", [(2, 5, 2, 128), (3, 17, 3, 64), (2, 65, 3, 64), (1, 257, 6, 128)])
def test_attention_bound_admits_fp32_and_rejects_a_shifted_value_row(shape, steepest):
    """The elementwise bound the GPU test holds the kernel to under 30x larger q (near-one-hot softmax): torch's own fp32 attention on
    the CPU (relative bias) is inside it, an attention that pairs every weight with the NEXT key's value row is at least 100x outside."""
    B, T, H, hd = shape
    x = R.attention_inputs(B, T, H, hd, seed=sum(shape), q_gain=30.0)
    D = H * hd
    q, k, v = x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D]
    slopes = torch.full((H,), R.STEEPEST) if steepest else R.hf_slopes(H)
    ref = R.alibi_attention_ref(q, k, v, slopes, B, T, H, hd, 1.0)
    bound = R.alibi_attention_bound(q, k, v, slopes, B, T, H, hd, 1.0)
    inside = worst_ratio(R.alibi_attention_ref(q, k, v, slopes, B, T, H, hd, 1.0, dtype=torch.float32), ref, bound)
    wrong = worst_ratio(R.alibi_attention_ref(q, k, v, slopes, B, T, H, hd, 1.0, v_shift=1), ref, bound)
    print(f"alibi attention bound {shape} {'steepest' if steepest else 'bloom'}: torch fp32 at {inside:.3f} of it, shifted value rows at {wrong:.1e}, "
          f"bound max {bound.max().item():.2e}")
    assert inside <= 1.0 and wrong >= 100.0


@pytest.mark.parametrize("D", [132, 2560, 8192])
def test_offset_row_bound_admits_fp32_and_rejects_the_one_pass_variance(D):
    """Rows of unit spread around 1e4: torch's own fp32 F.layer_norm is inside layernorm_bound, E[x^2] - E[x]^2 in fp32 is at least 100x
    outside it (1e8 has an ulp of 8: the variance of 1 is lost)."""
    g = torch.Generator().manual_seed(D)
    x = torch.randn((4, D), generator=g) + 1e4
    gamma, beta = 1.0 + 0.3 * torch.randn((D,), generator=g), 0.3 * torch.randn((D,), generator=g)
    ref = R.layernorm_ref(x, gamma, beta, 1e-5)
    bound = R.layernorm_bound(x, gamma, beta, 1e-5)
    inside = worst_ratio(torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-5), ref, bound)
    wrong = worst_ratio(R.layernorm_one_pass32(x, gamma, beta, 1e-5), ref, bound)
    print(f"offset-row layernorm bound D={D}: torch fp32 at {inside:.3f} of it, one-pass variance at {wrong:.1e}, bound max {bound.max().item():.2e}")
    assert inside <= 1.0 and wrong >= 100.0
