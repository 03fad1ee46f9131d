"""LLaMA-family text encoder, the part that needs no GPU: the two C entry points are exported, bound and refuse bad arguments on the
host; HipLlamaModel refuses every config it does not cover, naming the field; and tests/llama_refs.py — the float64 formulas the GPU
tests lean on — IS HF's LlamaModel (eager, fp32), whose own features do not depend on right padding."""
import ctypes
import os

import pytest
import torch

import llama_refs as L
from op_refs import worst_ratio
from util import rel_err


@pytest.fixture(scope="module")
def lib():
    from mertools_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mertools_amd import build
        build.build()
    return _lib.lib()


@pytest.fixture(scope="module", params=sorted(L.TINY))
def tiny(request):
    return request.param, L.tiny_llama(request.param)


def test_entry_points_are_exported_and_bound(lib):
    from mertools_amd import _lib, ops
    for name in ("mer_rmsnorm", "mer_rope_attention"):
        assert hasattr(lib, name) and name in _lib._PROTOS, name
        assert name in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mer_hip.h")).read()
    assert callable(ops.rmsnorm) and callable(ops.rope_attention)


def test_bad_arguments_fail_on_the_host(lib):
    """The pointers are host memory and are never dereferenced: every refusal is decided before a launch."""
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    f = ctypes.c_float
    ok_norm = dict(x=p, ldx=8, gamma=None, eps=f(1e-6), M=1, D=8, out32=p, ld32=8, hi=None, lo=None, ld16=8, dtype=0)

    def norm(**kw):
        a = dict(ok_norm, **kw)
        return lib.mer_rmsnorm(a["x"], a["ldx"], a["gamma"], a["eps"], a["M"], a["D"], a["out32"], a["ld32"], a["hi"], a["lo"], a["ld16"], a["dtype"], None)
    for kw in (dict(D=6, ldx=8), dict(D=8196, ldx=8196, ld32=8196), dict(x=None), dict(M=0), dict(out32=None), dict(dtype=2), dict(ldx=4)):
        assert norm(**kw) < 0, kw
        assert b"mer_rmsnorm" in lib.mer_last_error(), (kw, lib.mer_last_error())
    ok_att = dict(q=p, k=p, v=p, ld=384, cos=p, sin=p, hi=p, lo=None, ldo=128, B=1, T=4, H=1, hd=128, dtype=0)

    def att(**kw):
        a = dict(ok_att, **kw)
        return lib.mer_rope_attention(a["q"], a["k"], a["v"], a["ld"], a["cos"], a["sin"], a["hi"], a["lo"], a["ldo"], a["B"], a["T"], a["H"], a["hd"],
                                      f(1.0), a["dtype"], None)
    for kw in (dict(hd=72), dict(T=0), dict(T=2049), dict(cos=None), dict(sin=None), dict(q=None), dict(hi=None), dict(B=0), dict(H=0), dict(ld=100),
               dict(ldo=64), dict(hd=32), dict(hd=256), dict(dtype=3), dict(q=p + 4)):
        assert att(**kw) < 0, kw
        assert b"mer_rope_attention" in lib.mer_last_error(), (kw, lib.mer_last_error())


def _config(**kw):
    import transformers as tr
    base = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, intermediate_size=688, num_hidden_layers=1, vocab_size=32)
    base.update(kw)
    return tr.LlamaConfig(**base)


@pytest.mark.parametrize("field,make", [
    ("model_type", lambda: __import__("transformers").MistralConfig(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, intermediate_size=688,
                                                                    num_hidden_layers=1, vocab_size=32)),
    ("hidden_act", lambda: _config(hidden_act="gelu")),
    ("attention_bias", lambda: _config(attention_bias=True)),
    ("mlp_bias", lambda: _config(mlp_bias=True)),
    ("num_key_value_heads", lambda: _config(num_key_value_heads=1)),
    ("head_dim", lambda: _config(hidden_size=192, num_attention_heads=2, num_key_value_heads=2)),          # head_dim 96
    ("head_dim", lambda: _config(hidden_size=256, num_attention_heads=8, num_key_value_heads=8)),          # head_dim 32
    ("rope_type", lambda: _config(rope_parameters={"rope_type": "linear", "factor": 2.0, "rope_theta": 10000.0})),
    ("hidden_size", lambda: _config(hidden_size=132, num_attention_heads=2, num_key_value_heads=2, head_dim=64)),
    ("intermediate_size", lambda: _config(intermediate_size=684)),
])
def test_unsupported_configs_are_refused_by_name(field, make):
    """Refused at construction, before a weight is read (the state dict is empty) and before the library or a GPU is needed."""
    from mertools_amd.llama import HipLlamaModel, check_config
    cfg = make()
    with pytest.raises(ValueError, match=field) as ei:
        HipLlamaModel({}, cfg, device="cpu")
    value = {"rope_type": "linear", "model_type": cfg.model_type}.get(field, getattr(cfg, field, None))
    assert str(value) in str(ei.value), ei.value
    with pytest.raises(ValueError, match=field):
        check_config(cfg)


def test_supported_config_passes_the_check():
    from mertools_amd.llama import check_config
    assert check_config(_config()) == (256, 2, 128, 688, 1, 10000.0)
    assert check_config(_config(hidden_size=128, intermediate_size=344))[:3] == (128, 2, 64)


def test_float64_forward_is_the_hf_module(tiny):
    name, m = tiny
    ids = L.batch_ids(lengths=(17,))
    ref = L.hf_hidden_states(m, ids)
    got = L.llama_forward64(m.state_dict(), m.config, ids)
    assert len(got) == len(ref) == m.config.num_hidden_layers + 1
    worst = max(rel_err(r, g)[0] for r, g in zip(ref, got))
    print(f"llama_forward64 vs HF fp32 [{name}]: worst hidden state {worst:.2e}")
    assert worst <= 5e-6


def test_hf_features_do_not_depend_on_right_padding(tiny):
    """Sentence 1 (9 tokens) alone against the same sentence inside the right-padded batch of three (17 tokens), on the HF module."""
    name, m = tiny
    ids = L.batch_ids()
    n = L.LENGTHS[1]
    mask = (torch.arange(ids.shape[1])[None] < torch.tensor(L.LENGTHS)[:, None]).long()
    fr_b = torch.stack(L.hf_hidden_states(m, ids, mask))[[-4, -3, -2, -1]].sum(0)[1, :n]
    fr_a, utt_a = L.hf_sentence_features(m, ids[1], n)
    e_fr, e_utt = rel_err(fr_b, fr_a)[0], rel_err(fr_b.mean(0), utt_a)[0]
    print(f"HF batch vs alone [{name}]: FRAME {e_fr:.2e} UTT {e_utt:.2e}")
    assert e_fr <= 5e-6 and e_utt <= 5e-6


@pytest.mark.parametrize("shape", [(2, 5, 2, 128), (3, 17, 2, 128), (2, 65, 3, 64), (1, 257, 2, 128)])
def test_attention_bound_admits_fp32_and_rejects_a_shifted_value_row(shape):
    """The elementwise bound the GPU test holds the kernel to under 30x larger q (near-one-hot softmax): torch's own fp32 attention on
    the CPU is inside it, an attention that pairs every weight with the NEXT key's value row is at least 100x outside."""
    B, T, H, hd = shape
    x = L.attention_inputs(B, T, H, hd, seed=sum(shape), q_gain=30.0)
    D = H * hd
    q, k, v = x[:, :D], x[:, D:2 * D], x[:, 2 * D:3 * D]
    cos, sin = L.rope_tables(T, hd)
    ref = L.rope_attention_ref(q, k, v, cos, sin, B, T, H, hd, 1.0)
    bound = L.rope_attention_bound(q, k, v, cos, sin, B, T, H, hd, 1.0)
    inside = worst_ratio(L.rope_attention_ref(q, k, v, cos, sin, B, T, H, hd, 1.0, dtype=torch.float32), ref, bound)
    wrong = worst_ratio(L.rope_attention_ref(q, k, v, cos, sin, B, T, H, hd, 1.0, v_shift=1), ref, bound)
    print(f"rope attention bound {shape}: torch fp32 at {inside:.3f} of it, shifted value rows at {wrong:.1e}, bound max {bound.max().item():.2e}")
    assert inside <= 1.0 and wrong >= 100.0
