"""LMF (toolkit.models.lmf.LMF over mer_lmf_fwd / mer_lmf_bwd) — everything that needs no GPU: registry, state_dict and initial
values against the reference module's own (tests/golden/fusion_lmf.npz, gen_golden_lmf.py), the tuning grid, the group
engines' scope, the C ABI and its argument validation."""
import argparse
import ctypes
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _args(**kw):
    a = dict(model="lmf", audio_dim=48, text_dim=40, video_dim=32, hidden_dim=32, rank=4, output_dim1=6, output_dim2=1, dropout=0.0,
             grad_clip=-1.0, feat_type="utt")
    a.update(kw)
    return argparse.Namespace(**a)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "fusion_lmf.npz"))


@pytest.fixture(scope="module")
def lib():
    from mertools_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from mertools_amd import build
        build.build()
    return _lib.lib()


@pytest.mark.parametrize("feat_type,prefix,seed", [("utt", "", 1237), ("frm_align", "frm_", 4321)])
def test_lmf_builds_with_the_reference_state_dict_and_initial_values(gold, feat_type, prefix, seed):
    from mertools_amd.toolkit.models import get_models
    from mertools_amd.toolkit.models.lmf import LMF
    torch.manual_seed(seed)
    m = get_models(_args(feat_type=feat_type))
    assert isinstance(m.model, LMF) and m.model.grad_clip == -1.0 and not next(m.parameters()).is_cuda
    assert isinstance(m.model.post_fusion_dropout, torch.nn.Dropout)
    keys = sorted(k[len(prefix + "init_"):] for k in gold.files if k.startswith(prefix + "init_"))
    sd = m.model.state_dict()
    assert sorted(sd) == keys
    if feat_type == "utt":
        assert len(sd) == 27
    for k, v in sd.items():
        want = gold[prefix + "init_" + k]
        assert tuple(v.shape) == want.shape, k
        assert np.array_equal(v.numpy(), want), f"{k}: initial values differ from the reference's under the same seed"
    assert tuple(sd["audio_factor"].shape) == (4, 33, 16) and tuple(sd["fusion_weights"].shape) == (1, 4)
    assert tuple(sd["fusion_bias"].shape) == (1, 16) and not sd["fusion_bias"].any()
    # parameter order (what an optimiser and the flat buffer of FusionGraphTrainer see) is the reference's
    assert [k for k, _ in m.model.named_parameters()] == [k[len(prefix + "grad0_"):] for k in gold.files if k.startswith(prefix + "grad0_")]


def test_other_baselines_still_raise():
    from mertools_amd.toolkit.models import get_models
    for name in ("tfn", "misa", "mmim", "mfn", "graph_mfn", "mfm", "mctn", "mult", "ef_lstm"):
        with pytest.raises(NotImplementedError):
            get_models(_args(model=name))


def test_tuning_grid_and_rank_reach_args(tmp_path):
    import yaml
    from mertools_amd.toolkit.utils.functions import func_random_select, merge_args_config
    with open(os.path.join(ROOT, "mertools_amd", "toolkit", "model-tune.yaml")) as fh:
        grid = yaml.safe_load(fh)["lmf"]
    assert grid == {"hidden_dim": [32, 64, 128, 256], "dropout": [0.2, 0.3, 0.4, 0.5], "rank": [3, 4, 5, 6], "grad_clip": [-1.0],
                    "lr": [1.0e-3, 1.0e-4]}
    assert all(isinstance(v, float) for v in grid["lr"])
    random.seed(3)
    args = merge_args_config(argparse.Namespace(model="lmf", lr=None, hidden_dim=None), func_random_select(dict(grid)))
    assert isinstance(args.rank, int) and args.rank in (3, 4, 5, 6) and args.hidden_dim in (32, 64, 128, 256)
    # --hyper_path: main_release._setup reads the file's entry as it stands
    from mertools_amd import main_release
    hyper = tmp_path / "tune.yaml"
    hyper.write_text("lmf:\n  hidden_dim: 64\n  dropout: 0.0\n  rank: 5\n  grad_clip: -1.0\n  lr: 1.0e-3\n")
    a = main_release.build_parser().parse_args(["--model", "lmf", "--feat_type", "utt", "--dataset", "MER2023", "--audio_feature", "a-UTT",
                                                "--text_feature", "t-UTT", "--video_feature", "v-UTT", "--hyper_path", str(hyper),
                                                "--save_root", str(tmp_path / "saved")])
    a, *_ = main_release._setup(a)
    assert a.rank == 5 and isinstance(a.rank, int) and a.hidden_dim == 64 and a.lr == 1e-3


def test_group_engines_still_refuse_lmf():
    from mertools_amd import main_release
    a = main_release.build_parser().parse_args(["--model", "lmf", "--feat_type", "utt", "--dataset", "MER2023", "--parallel_folds", "--seed", "0"])
    with pytest.raises(ValueError, match="--model lmf"):
        main_release.check_group_scope(a)
    with pytest.raises(ValueError, match="--model attention --feat_type utt --dataset MER2023"):
        main_release.main(["--model", "lmf", "--feat_type", "utt", "--dataset", "MER2023", "--audio_feature", "a-UTT", "--text_feature", "t-UTT",
                           "--video_feature", "v-UTT", "--parallel_folds", "--seed", "0"])


def test_lmf_entry_points_are_exported_and_bound(lib):
    from mertools_amd import _lib
    for name in ("mer_lmf_fwd", "mer_lmf_bwd", "mer_lmf_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib._PROTOS, name
    assert len(_lib._PROTOS["mer_lmf_fwd"][1]) == 15 and len(_lib._PROTOS["mer_lmf_bwd"][1]) == 24
    assert lib.mer_lmf_workspace_bytes(32, 128, 4, 64) >= 0
    assert lib.mer_lmf_workspace_bytes(2048, 1024, 16, 512) >= 0 and lib.mer_lmf_workspace_bytes(1, 1, 1, 1) >= 0


BAD_SHAPES = [dict(R=0), dict(R=17), dict(H=0), dict(H=1025), dict(O=0), dict(O=513), dict(B=0), dict(B=2049)]


@pytest.mark.parametrize("bad", BAD_SHAPES + [dict(null=True)], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_lmf_bad_arguments_fail_loudly_without_a_gpu(lib, bad):
    """A bad shape or a NULL required pointer is refused before anything touches a GPU (this test runs without one): the
    pointers handed over are host addresses that a launch would fault on."""
    s = dict(B=32, H=64, R=4, O=32)
    s.update({k: v for k, v in bad.items() if k != "null"})
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = "null" in bad
    shape = (s["B"], s["H"], s["R"], s["O"])
    rc = lib.mer_lmf_fwd(p, p, p, p, p, p, p, p, *shape, None, None if null else p, None)
    assert rc < 0 and b"mer_lmf_fwd" in lib.mer_last_error(), (rc, lib.mer_last_error())
    rc = lib.mer_lmf_bwd(p, p, p, p, p, p, p, p, p, *shape, None, None, None, p, p, None if null else p, p, p, None, 0, None)
    assert rc < 0 and b"mer_lmf_bwd" in lib.mer_last_error(), (rc, lib.mer_last_error())
    if null:
        rc = lib.mer_lmf_bwd(p, p, p, p, p, p, p, p, None, *shape, None, None, None, p, p, p, p, p, None, 0, None)   # proj
        assert rc < 0 and b"mer_lmf_bwd" in lib.mer_last_error()
    else:
        rc = lib.mer_lmf_workspace_bytes(*shape)
        assert rc < 0 and b"mer_lmf_workspace_bytes" in lib.mer_last_error(), (rc, lib.mer_last_error())


def test_fp32_reference_sits_well_inside_the_bars(gold):
    """The bars of tests/test_lmf_gpu.py's model tests (2e-5 forward, 5e-5 gradients; 5e-4 for the frame-level gradients) are
    only meaningful if the fp32 reference itself is far closer than that to the exact values: its distance from the float64
    twin (f64diff_* = twin - fp32, gen_golden_lmf.py) must stay under a quarter of each bar, in util.assert_close's norm."""
    from util import rel_err
    for prefix, gbar in (("", 5e-5), ("frm_", 5e-4)):
        worst, seen = 0.0, 0
        for key in gold.files:
            if not key.startswith(prefix + "f64diff_"):
                continue
            name = prefix + key[len(prefix + "f64diff_"):]
            v32 = torch.from_numpy(gold[name])
            seen += 1
            v64 = v32.double() + torch.from_numpy(gold[key]).double()
            e, _ = rel_err(v32, v64)
            bar = 2e-5 if "_out_" in key else gbar
            worst = max(worst, e / bar)
            assert e <= bar / 4, f"{name}: the fp32 reference is {e:.2e} from its float64 twin, bar {bar:.0e}"
        assert seen == 3 + 27, (prefix, seen)   # three forward outputs and every parameter's first-step gradient
        print(f"{prefix or 'utt_'}: worst fp32-vs-fp64 distance = {worst:.3f} of its bar")
