"""LMF on the HIP kernels (mer_lmf_fwd / mer_lmf_bwd through fusion_ops.lmf_fuse, toolkit.models.lmf.LMF, FusionGraphTrainer,
main_release --model lmf) against float64 torch and against vectors made by the reference's own LMF module
(tests/golden/fusion_lmf.npz, gen_golden_lmf.py).  Bars: the project's fp32 bars of tests/test_fusion_gpu.py in
util.assert_close's norm — 2e-5 forward, 5e-5 gradients."""
import argparse
import os

import numpy as np
import pytest
import torch

from util import assert_close, rel_err

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_TOL, GRAD_TOL = 2e-5, 5e-5
NAMES = ("audio_h", "video_h", "text_h", "audio_factor", "video_factor", "text_factor", "fusion_weights", "fusion_bias")
SHAPES = [(1, 32, 3, 16), (32, 64, 4, 32), (33, 256, 6, 128), (7, 33, 5, 16), (2, 1, 1, 1), (257, 64, 4, 32)]


def _inputs(B, H, R, O, seed=0):
    """Order-one values everywhere, so that an error in one factor is not lost under the bias."""
    g = torch.Generator().manual_seed(1000 * seed + B + 7 * H + 13 * R + O)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    s = (H + 1) ** -0.5
    return [r(B, H), r(B, H), r(B, H), r(R, H + 1, O) * s, r(R, H + 1, O) * s, r(R, H + 1, O) * s, r(1, R), r(1, O)], r(B, O)


def _compose(ha, hv, ht, fa, fv, ft, w, bias):
    """The fusion written as ordinary torch ops: [1, h] @ F per modality and rank, their product, the rank-weighted sum, the bias."""
    one = torch.ones(ha.shape[0], 1, dtype=ha.dtype, device=ha.device)
    pa, pv, pt = (torch.matmul(torch.cat([one, h], 1), f) for h, f in ((ha, fa), (hv, fv), (ht, ft)))   # [R, B, O]
    return (w.reshape(-1, 1, 1) * (pa * pv * pt)).sum(0) + bias.reshape(1, -1)


def _run(fn, xs, dout, dev=None, dtype=torch.float64, grads=range(8)):
    xs = [x.detach().clone().to(dtype=dtype, device=dev).requires_grad_(i in grads) for i, x in enumerate(xs)]
    out = fn(*xs)
    out.backward(dout.to(dtype=dtype, device=dev))
    return out.detach(), [x.grad for x in xs]


# the edges of what the entry points accept: the largest H, R and O together (the forward's 64 KiB of LDS and 1024-thread
# blocks, 33 k'-tiles x 8 o-tiles x 16 ranks of factor-gradient blocks) and the largest B (128 row tiles, 2048-term sums over b)
LIMITS = [(3, 1024, 16, 512), (2048, 8, 2, 3)]


@pytest.mark.parametrize("B,H,R,O", SHAPES + LIMITS)
def test_lmf_fuse_matches_float64(dev, B, H, R, O):
    from mertools_amd.fusion_ops import lmf_fuse
    xs, dout = _inputs(B, H, R, O)
    want, gwant = _run(_compose, xs, dout)
    got32, ggot32 = _run(_compose, xs, dout, dtype=torch.float32)
    got, ggot = _run(lmf_fuse, xs, dout, dev=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, O)
    lines = []
    for name, a, c, w_, tol in [("out", got, got32, want, FWD_TOL)] + [("d" + n, a, c, w_, GRAD_TOL) for n, a, c, w_ in zip(NAMES, ggot, ggot32, gwant)]:
        assert a.shape == w_.shape, name
        lines.append(f"{name}: hip {rel_err(a, w_)[0]:.2e}  fp32 torch (cpu) {rel_err(c, w_)[0]:.2e}  bar {tol:.0e}")
    print(f"\n(B,H,R,O)=({B},{H},{R},{O})\n  " + "\n  ".join(lines))
    # the inputs must leave the bars meaningful: plain fp32 torch has to sit within a quarter of each (else change the seed / scales, not the bar)
    assert rel_err(got32, want)[0] <= FWD_TOL / 4
    for n, c, w_ in zip(NAMES, ggot32, gwant):
        assert rel_err(c, w_)[0] <= GRAD_TOL / 4, n
    assert_close(got.cpu(), want, FWD_TOL, "lmf_fuse out")
    for n, a, w_ in zip(NAMES, ggot, gwant):
        assert_close(a.cpu(), w_, GRAD_TOL, "lmf_fuse d" + n)


def test_lmf_fuse_rows_are_independent_and_runs_are_bit_identical(dev):
    from mertools_amd.fusion_ops import lmf_fuse
    B, H, R, O = 33, 256, 6, 128
    xs, dout = _inputs(B, H, R, O, seed=1)
    xd = [x.float().to(dev) for x in xs]
    with torch.no_grad():
        full = lmf_fuse(*xd)
        for row in (5, 32):   # inside a row tile, and alone in the ragged last one
            one = lmf_fuse(*(x[row:row + 1] for x in xd[:3]), *xd[3:])
            assert (full[row] - one[0]).abs().max().item() == 0.0, row
    o1, g1 = _run(lmf_fuse, xs, dout, dev=dev, dtype=torch.float32)
    o2, g2 = _run(lmf_fuse, xs, dout, dev=dev, dtype=torch.float32)
    assert torch.equal(o1, o2) and torch.equal(o1, full)
    for n, a, b in zip(NAMES, g1, g2):
        assert torch.equal(a, b), f"d{n} differs between two runs on the same inputs"
    # no gradient wanted for the encoder outputs (dh* = NULL): the five parameter gradients keep their bits
    o3, g3 = _run(lmf_fuse, xs, dout, dev=dev, dtype=torch.float32, grads=range(3, 8))
    assert g3[0] is None and g3[1] is None and g3[2] is None
    for n, a, b in zip(NAMES[3:], g1[3:], g3[3:]):
        assert torch.equal(a, b), f"d{n} changes when dh is not asked for"
    # only one of them
    o4, g4 = _run(lmf_fuse, xs, dout, dev=dev, dtype=torch.float32, grads=(1, 3, 4, 5, 6, 7))
    assert g4[0] is None and g4[2] is None and torch.equal(g4[1], g1[1])


def test_lmf_fuse_overwrites_gradients_and_refuses_bad_input(dev):
    """Gradient buffers are overwritten, never accumulated into (pre-filled with NaN here); shape mismatches and CPU tensors raise."""
    from mertools_amd import _lib
    from mertools_amd.fusion_ops import lmf_fuse
    from mertools_amd.ops import _p, stream
    B, H, R, O = 7, 33, 5, 16
    xs, dout = _inputs(B, H, R, O, seed=2)
    want, gwant = _run(_compose, xs, dout)
    ha, hv, ht, fa, fv, ft, w, bias = (x.float().to(dev) for x in xs)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)   # noqa: E731
    proj, out = nan(3, R, B, O), nan(B, O)
    lib = _lib.lib()
    assert lib.mer_lmf_workspace_bytes(B, H, R, O) == 0
    _lib.check(lib.mer_lmf_fwd(_p(ha), _p(hv), _p(ht), _p(fa), _p(fv), _p(ft), _p(w), _p(bias), B, H, R, O, _p(proj), _p(out), stream()), "fwd")
    out2 = nan(B, O)
    _lib.check(lib.mer_lmf_fwd(_p(ha), _p(hv), _p(ht), _p(fa), _p(fv), _p(ft), _p(w), _p(bias), B, H, R, O, None, _p(out2), stream()), "fwd")
    assert torch.equal(out, out2) and torch.isfinite(proj).all()
    outs = [nan(B, H), nan(B, H), nan(B, H), nan(R, H + 1, O), nan(R, H + 1, O), nan(R, H + 1, O), nan(R), nan(O)]
    _lib.check(lib.mer_lmf_bwd(_p(dout.float().to(dev)), _p(ha), _p(hv), _p(ht), _p(fa), _p(fv), _p(ft), _p(w), _p(proj), B, H, R, O,
                               *(_p(t) for t in outs), None, 0, stream()), "bwd")
    torch.cuda.synchronize()
    assert_close(out.cpu(), want, FWD_TOL, "out")
    for n, a, w_ in zip(NAMES, outs, gwant):
        assert_close(a.cpu().reshape(w_.shape), w_, GRAD_TOL, "d" + n)
    with pytest.raises(_lib.MerError):
        lmf_fuse(ha, hv, ht, fa, fv, ft[:, :-1], w, bias)
    # a tensor of the wrong rank is named by the same message, not by a failed unpacking
    with pytest.raises(_lib.MerError, match="lmf_fuse: shapes"):
        lmf_fuse(ha[0], hv[0], ht[0], fa, fv, ft, w, bias)
    with pytest.raises(_lib.MerError, match="lmf_fuse: shapes"):
        lmf_fuse(ha, hv, ht, fa[0], fv[0], ft[0], w, bias)
    with pytest.raises(_lib.MerError):
        lmf_fuse(ha.cpu(), hv, ht, fa, fv, ft, w, bias)


# ---- the model against the reference's own module ----
def _args(feat_type="utt", dropout=0.0):
    return argparse.Namespace(model="lmf", audio_dim=48, text_dim=40, video_dim=32, hidden_dim=32, rank=4, output_dim1=6, output_dim2=1,
                              dropout=dropout, grad_clip=-1.0, feat_type=feat_type)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "fusion_lmf.npz"))


def _model(gold, dev, feat_type="utt", prefix=""):
    from mertools_amd.toolkit.models import get_models
    m = get_models(_args(feat_type))
    m.model.load_state_dict({k: torch.from_numpy(gold[prefix + "init_" + k]) for k in m.model.state_dict()})
    return m.to(dev)


def test_lmf_forward_matches_reference(dev, gold):
    m = _model(gold, dev).eval()
    batch = {k: torch.from_numpy(gold["x_" + k][0]).to(dev) for k in ("audios", "texts", "videos")}
    with torch.no_grad():
        f, e, v, il = m(batch)
    torch.cuda.synchronize()
    assert tuple(f.shape) == (32, 16)
    assert_close(f.cpu(), torch.from_numpy(gold["out_features"]), FWD_TOL, "features")
    assert_close(e.cpu(), torch.from_numpy(gold["out_emos_out"]), FWD_TOL, "emos_out")
    assert_close(v.cpu(), torch.from_numpy(gold["out_vals_out"]), FWD_TOL, "vals_out")
    assert il.dtype == torch.int64 and il.ndim == 0 and int(il) == 0 and il.is_cuda


@pytest.mark.parametrize("opt", ["torch_adam", "hip_adam"])
def test_lmf_training_steps_match_reference(dev, gold, opt):
    """The assertions of test_fusion_gpu.test_attention_training_steps_match_reference for the LMF model: first-step gradients,
    per-step losses, final parameters after 5 Adam steps."""
    from mertools_amd.fusion_ops import HipAdam
    from mertools_amd.toolkit.utils.loss import CELoss, MSELoss
    g = gold
    m = _model(g, dev).train()
    cls_loss, reg_loss = CELoss(), MSELoss()
    o = (HipAdam if opt == "hip_adam" else torch.optim.Adam)(m.parameters(), lr=1e-3, weight_decay=1e-5)
    steps = len(g["losses"])
    for s in range(steps):
        o.zero_grad()
        batch = {k: torch.from_numpy(g["x_" + k][s]).to(dev) for k in ("audios", "texts", "videos")}
        f, e, v, il = m(batch)
        loss = il + cls_loss(e, torch.from_numpy(g["emos"][s]).to(dev)) + reg_loss(v, torch.from_numpy(g["vals"][s]).to(dev))
        loss.backward()
        if s == 0:
            for k, p in m.model.named_parameters():
                assert_close(p.grad.cpu(), torch.from_numpy(g["grad0_" + k]), GRAD_TOL, f"grad {k}")
        o.step()
        assert abs(loss.item() - g["losses"][s]) <= 5e-5 * abs(g["losses"][s]), (s, loss.item(), g["losses"][s])
    torch.cuda.synchronize()
    for k, p in m.model.state_dict().items():
        assert_close(p.cpu(), torch.from_numpy(g["final_" + k]), 1e-4, f"final {k}")


def test_lmf_frame_level_matches_reference(dev, gold):
    """feat_type='frm_align' (three LSTMEncoders): forward and first-step gradients at the bars of
    test_fusion_gpu.test_attention_model_frame_level_matches_reference (2e-5 outputs, 5e-4 gradients)."""
    from mertools_amd.toolkit.utils.loss import CELoss, MSELoss
    g = gold
    m = _model(g, dev, "frm_align", "frm_").train()
    batch = {k: torch.from_numpy(g["frm_x_" + k]).to(dev) for k in ("audios", "texts", "videos")}
    f, e, v, il = m(batch)
    loss = il + CELoss()(e, torch.from_numpy(g["frm_emos"]).to(dev)) + MSELoss()(v, torch.from_numpy(g["frm_vals"]).to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert_close(f.detach().cpu(), torch.from_numpy(g["frm_out_features"]), 2e-5, "frame-level features")
    assert_close(e.detach().cpu(), torch.from_numpy(g["frm_out_emos_out"]), 2e-5, "frame-level emos_out")
    assert_close(v.detach().cpu(), torch.from_numpy(g["frm_out_vals_out"]), 2e-5, "frame-level vals_out")
    assert abs(loss.item() - float(g["frm_loss"])) <= 5e-5 * abs(float(g["frm_loss"]))
    for k, p in m.model.named_parameters():
        assert_close(p.grad.cpu(), torch.from_numpy(g["frm_grad0_" + k]), 5e-4, f"grad {k}")


def test_lmf_graph_trainer_equals_eager_bitwise(dev, gold):
    """FusionGraphTrainer on an LMF model: the captured-and-replayed step and the same step launched eagerly give the same bits
    (losses, every parameter), also through a second, ragged minibatch size; eval_step equals a plain no_grad forward."""
    from mertools_amd.fusion_trainer import FusionGraphTrainer
    g = gold
    runs = []
    for use_graph in (True, False):
        m = _model(g, dev)
        tr = FusionGraphTrainer(m, lr=1e-3, weight_decay=1e-5, grad_clip=-1.0, use_graph=use_graph)
        losses = []
        for s in (0, 1, 2, 3, 4):
            n = 5 if s in (3, 4) else 32    # B = 5: the ragged last minibatch of an epoch (a second capture), replayed twice
            batch = {k: torch.from_numpy(g["x_" + k][s][:n]).to(dev) for k in ("audios", "texts", "videos")}
            loss, e, v = tr.train_step(batch, torch.from_numpy(g["emos"][s][:n]).to(dev), torch.from_numpy(g["vals"][s][:n]).to(dev))
            losses.append(loss.item())
        batch = {k: torch.from_numpy(g["x_" + k][0]).to(dev) for k in ("audios", "texts", "videos")}
        loss, e, v = tr.eval_step(batch, torch.from_numpy(g["emos"][0]).to(dev), torch.from_numpy(g["vals"][0]).to(dev))
        e, v = e.clone(), v.clone()
        with torch.no_grad():
            _, e2, v2, _ = m.eval()(batch)
        assert torch.equal(e, e2) and torch.equal(v, v2), f"eval_step differs from a no_grad forward (graph={use_graph})"
        runs.append((losses, tr.flat.clone(), e, v))
    assert np.isfinite(runs[0][0]).all()
    np.testing.assert_allclose(runs[0][0][:3], g["losses"][:3], rtol=5e-5)     # the first three are the reference's steps
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


def _corpus(tmp_path, seed):
    """A small synthetic MER2023-shaped corpus (label npz + per-clip UTT .npy files), as tests/test_fusion_gpu.py's driver tests build it."""
    root = tmp_path / "data" / "mer2023-dataset-process"
    rng = np.random.RandomState(seed)
    names = {"train": [f"tr_{i:03d}" for i in range(50)], "test1": [f"t1_{i:02d}" for i in range(9)],
             "test2": [f"t2_{i:02d}" for i in range(7)], "test3": [f"t3_{i:02d}" for i in range(5)]}
    emos = ['neutral', 'angry', 'happy', 'sad', 'worried', 'surprise']
    corp = {}
    for split, ns in names.items():
        corp[f"{split}_corpus"] = {n: {"emo": emos[rng.randint(6)], "val": float(rng.uniform(-3, 3))} for n in ns}
        if split == "test3":
            for n in ns:
                del corp[f"{split}_corpus"][n]["val"]
    os.makedirs(root / "features", exist_ok=True)
    np.savez_compressed(root / "label-6way.npz", **{k: np.array(v, dtype=object) for k, v in corp.items()})
    for feat, d in {"audio-UTT": 24, "text-UTT": 16, "video-UTT": 20}.items():
        os.makedirs(root / "features" / feat, exist_ok=True)
        for ns in names.values():
            for n in ns:
                np.save(root / "features" / feat / f"{n}.npy", rng.randn(d).astype(np.float32))
    return tmp_path / "data"


def test_main_release_lmf(dev, tmp_path):
    """python -m mertools_amd.main_release --model lmf on the synthetic corpus: a run on the tuning grid finishes and writes its
    result files with `rank` among the saved args; with dropout forced to 0 through --hyper_path the graph-replayed loop and
    --eager report the same metrics."""
    from mertools_amd import main_release
    data = _corpus(tmp_path, 2)
    base = ["--model", "lmf", "--feat_type", "utt", "--dataset", "MER2023", "--audio_feature", "audio-UTT", "--text_feature", "text-UTT",
            "--video_feature", "video-UTT", "--epochs", "2", "--batch_size", "16", "--gpu", "0", "--seed", "7", "--data_root", str(data)]
    res = main_release.main(base + ["--save_root", str(tmp_path / "grid")])
    assert len(res) == 5
    for fold in res:
        for k, x in fold.items():
            if isinstance(x, np.ndarray) and x.dtype.kind == "f":
                assert np.isfinite(x).all(), k
    saved = os.listdir(tmp_path / "grid-trimodal" / "result")
    assert sum(f.startswith("cv_") for f in saved) == 1 and sum(f.startswith("test1_") for f in saved) == 1
    cv = [f for f in saved if f.startswith("cv_")][0]
    assert "_model:lmf+utt+" in cv
    a = np.load(tmp_path / "grid-trimodal" / "result" / cv, allow_pickle=True)["args"].item()
    assert a.model == "lmf" and isinstance(a.rank, int) and a.rank in (3, 4, 5, 6) and a.hidden_dim in (32, 64, 128, 256)

    hyper = tmp_path / "tune.yaml"
    hyper.write_text("lmf:\n  hidden_dim: 64\n  dropout: 0.0\n  rank: 4\n  grad_clip: -1.0\n  lr: 1.0e-3\n")   # (dropout draws come from different RNG paths in the two loops)
    res_g = main_release.main(base + ["--hyper_path", str(hyper), "--save_root", str(tmp_path / "graph")])
    res_e = main_release.main(base + ["--hyper_path", str(hyper), "--save_root", str(tmp_path / "eager"), "--eager"])
    assert len(res_g) == len(res_e) == 5
    for fa, fb in zip(res_g, res_e):
        assert set(fa) == set(fb)
        for k in fa:
            if isinstance(fa[k], np.ndarray) and fa[k].dtype.kind == "f":
                assert fa[k].shape == fb[k].shape and np.allclose(fa[k], fb[k], rtol=2e-4, atol=2e-5), k
            elif isinstance(fa[k], list):
                assert fa[k] == fb[k], k     # clip names: same order
            elif k.endswith(("emoacc", "emofscore")):
                assert fa[k] == fb[k], (k, fa[k], fb[k])
            elif k.endswith("valmse"):
                assert np.isclose(fa[k], fb[k], rtol=2e-4), (k, fa[k], fb[k])
    strip = lambda f: f.rsplit("_", 1)[0]   # noqa: E731  (drop the time stamp)
    fg = sorted(strip(f) for f in os.listdir(tmp_path / "graph-trimodal" / "result"))
    fe = sorted(strip(f) for f in os.listdir(tmp_path / "eager-trimodal" / "result"))
    assert fg == fe, (fg, fe)
