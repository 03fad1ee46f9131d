"""Grouped Attention_TOPN training (csrc/fusion_topn_group.hip, mertools_amd.fusion_topn_group, main_release --parallel_folds /
--num_trials with --model attention_topn) on the GPU: the reference's golden steps, bitwise equality with the merged 3-stream
group, group invariance (position, idle models, group size) with dropout, the counter-based dropout masks, eval steps and the
CLI against the default sequential path."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch

from test_fusion_topn_group_cpu import base_argv, topn_corpus
from util import assert_close, rel_err

pytestmark = pytest.mark.gpu
G_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M64 = 0xFFFFFFFFFFFFFFFF
DIMS6 = (40, 24, 56, 33, 48, 72)
DIMS18 = (40, 24, 56, 33, 48, 72, 17, 64, 31, 96, 20, 45, 80, 9, 128, 51, 36, 67)


def _args(dims, H=32, dropout=0.0, grad_clip=-1.0, C2=0):
    return argparse.Namespace(model="attention_topn", audio_dim=list(dims), output_dim1=6, output_dim2=C2, dropout=dropout, hidden_dim=H,
                              grad_clip=grad_clip, feat_type="utt")


def _models(dev, n, seed, dims, **kw):
    from mertools_amd.toolkit.models import get_models
    torch.manual_seed(seed)
    return [get_models(_args(dims, **kw)).to(dev) for _ in range(n)]


def _tables(n, dims, seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(n, d, generator=g) for d in dims]
    return feats, torch.randint(0, 6, (n,), generator=g), (torch.rand(n, generator=g) * 6 - 3)


def _schedule(G, S, B, N, seed, partial=()):
    rng = np.random.RandomState(seed)
    index = rng.randint(0, N, size=(S, G, B)).astype(np.int32)
    count = np.full((S, G), B, dtype=np.int32)
    for g, n in partial:
        count[S - 1, g] = n
    return index, count


def test_topn_group_matches_golden_reference(dev):
    """A G=3 group, every slot loaded with tests/golden/fusion_attention_topn_train.npz's init_* (the reference's Attention_TOPN,
    6 streams of widths 40/24/56/33/48/72, H 32, emotion head only) and fed its 5 minibatches (lr 1e-3, wd 1e-5): the reference's
    losses at rtol 5e-5, its final parameters and its step-0 gradients at 1e-4 (test_group_matches_golden_reference's tolerances)."""
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer
    g = np.load(os.path.join(G_DIR, "fusion_attention_topn_train.npz"))
    dims, H = g["dims"].tolist(), int(g["hidden"])
    S, B = g["x_feat0"].shape[:2]
    tab = [torch.from_numpy(g[f"x_feat{i}"]).reshape(S * B, -1) for i in range(len(dims))]
    index = np.tile((np.arange(S)[:, None] * B + np.arange(B)[None, :])[:, None, :], (1, 3, 1)).astype(np.int32)
    for steps in (1, S):
        ms = _models(dev, 3, 0, dims, H=H)
        for m in ms:
            m.model.load_state_dict({k: torch.from_numpy(g["init_" + k]) for k in m.model.state_dict()})
        tr = FusionTopnGroupTrainer(ms, lr=1e-3, weight_decay=1e-5, grad_clip=-1.0, batch_size=B)
        tr.set_tables(tab, torch.from_numpy(g["emos"]).reshape(-1))
        loss, _, val = tr.run(index[:steps], np.full((steps, 3), B, dtype=np.int32), True)
        assert tuple(val.shape) == (steps, 3, B, 0)
        loss = loss.cpu().numpy()
        for k in range(3):
            print(f"slot {k} steps {steps}: loss rel err {np.abs(loss[:, k] / g['losses'][:steps] - 1).max():.3e}")
            np.testing.assert_allclose(loss[:, k], g["losses"][:steps], rtol=5e-5)
            if steps == 1:
                for name, p in ms[k].model.named_parameters():
                    if p.numel():
                        assert_close(p.grad.cpu(), torch.from_numpy(g["grad0_" + name]), 1e-4, f"slot {k} grad0 {name}")
            else:
                for name, p in ms[k].model.state_dict().items():
                    if p.numel() == 0:      # fc_out_2 of the emotion-only head
                        assert tuple(p.shape) == g["final_" + name].shape, name
                        continue
                    assert_close(p.cpu(), torch.from_numpy(g["final_" + name]), 1e-4, f"slot {k} final {name}")


def test_three_streams_bitwise_equal_the_merged_group(dev):
    """M = 3, C2 = 1, dropout 0: three models (different inits and lrs, one with grad_clip > 0), 20 steps, partial last batches:
    losses, emotion logits, valence outputs, final parameters, Adam moments and step counters are torch.equal to
    FusionGroupTrainer's on the same flat parameters (the two parameter layouts coincide for three streams) and minibatches.
    Both trainers run the one group engine, through two C ABIs: what this compares is the mer_fusion_group_* adapter's field
    mapping (Da, Dt, Dv -> D[0..2], feat_a, feat_t, feat_v -> feat[0..2], M = 3) against a descriptor stated directly."""
    from mertools_amd.fusion_group import FusionGroupTrainer
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer
    from mertools_amd.toolkit.models import get_models
    G, S, B, N, dims = 3, 20, 16, 300, (96, 80, 61)
    lrs, wds, clips = [1e-3, 3e-3, 5e-4], [1e-5, 0.0, 1e-4], [-1.0, 0.05, -1.0]
    att = []
    for k in range(G):
        torch.manual_seed(10 + k)
        att.append(get_models(argparse.Namespace(model="attention", audio_dim=dims[0], text_dim=dims[1], video_dim=dims[2], output_dim1=6,
                                                 output_dim2=1, dropout=0.0, hidden_dim=64, grad_clip=clips[k], feat_type="utt")).to(dev))
    top = [_models(dev, 1, 50 + k, dims, H=64, grad_clip=clips[k], C2=1)[0] for k in range(G)]
    feats, emos, vals = _tables(N, dims)
    index, count = _schedule(G, S, B, N, 1, partial=[(0, 5), (1, 11)])
    tr_a = FusionGroupTrainer(att, lr=lrs, weight_decay=wds, grad_clip=clips, batch_size=B)
    tr_t = FusionTopnGroupTrainer(top, lr=lrs, weight_decay=wds, grad_clip=clips, batch_size=B)
    assert tr_a.P == tr_t.P
    tr_t.flat.copy_(tr_a.flat)
    for a, t in zip(att, top):      # same flat layout: audio/text/video_encoder <-> encoder0/1/2, then the shared tail
        for (ka, pa), (kt, pt) in zip(a.model.state_dict().items(), t.model.state_dict().items()):
            assert ka.split(".", 1)[1] == kt.split(".", 1)[1] or ka == kt
            assert torch.equal(pa, pt), (ka, kt)
    tr_a.set_tables(*feats, emos, vals)
    tr_t.set_tables(feats, emos, vals)
    la, ea, va = (x.clone() for x in tr_a.run(index, count, True))
    lt, et, vt = (x.clone() for x in tr_t.run(index, count, True))
    assert torch.equal(la, lt)
    for k in range(G):
        for s in range(S):
            n = int(count[s, k])
            assert torch.equal(ea[s, k, :n], et[s, k, :n]) and torch.equal(va[s, k, :n], vt[s, k, :n, 0]), (k, s)
    for x in ("flat", "flat_grad", "m", "v", "step"):
        assert torch.equal(getattr(tr_a, x), getattr(tr_t, x)), x
    assert tr_t.step.tolist() == [S] * G


def _run_group(dev, inits, order, index, count, seeds, dims):
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer
    ms = [copy.deepcopy(inits[i]) for i in order]
    tr = FusionTopnGroupTrainer(ms, lr=[1e-3 * (1 + i) for i in order], weight_decay=1e-5, grad_clip=[0.1 if i % 2 else -1.0 for i in order],
                                seeds=[seeds[i] for i in order], batch_size=index.shape[2])
    feats, emos, vals = _tables(200, dims, seed=3)
    tr.set_tables(feats, emos, vals)
    loss, emo, val = (x.clone() for x in tr.run(index, count, True))
    return tr, loss, emo, val


@pytest.mark.parametrize("dims,C2", [(DIMS6, 0), (DIMS18, 1)], ids=["M6", "M18"])
def test_topn_group_invariance_with_dropout(dev, dims, C2):
    """Five models at dropout 0.3 (M = 6 emotion-only, M = 18 with the valence head; unequal widths, some odd): one group, five
    groups of one, and a permuted group in which models sit idle at some steps give each model bitwise the same losses, outputs,
    gradients, parameters, Adam moments and step counter; an idle step touches nothing."""
    G, S, B = 5, 8, 12
    inits = [_models(dev, 1, 20 + k, dims, dropout=0.3, C2=C2)[0] for k in range(G)]
    seeds = [(0x1234567 * (k + 1)) & M64 for k in range(G)]
    index, count = _schedule(G, S, B, 200, 5, partial=[(2, 7), (4, 1)])
    tr_a, la, ea, va = _run_group(dev, inits, list(range(G)), index, count, seeds, dims)
    singles = [_run_group(dev, inits, [k], index[:, k:k + 1], count[:, k:k + 1], seeds, dims) for k in range(G)]
    perm = [3, 0, 1, 4, 2]
    rng = np.random.RandomState(9)
    idle = {pos: set(rng.choice(S + 3, 3, replace=False).tolist()) for pos in range(G)}
    index_c = np.zeros((S + 3, G, B), dtype=np.int32)
    count_c = np.zeros((S + 3, G), dtype=np.int32)
    where = {}
    for pos, k in enumerate(perm):
        act = [s for s in range(S + 3) if s not in idle[pos]]
        for i, s in enumerate(act):
            index_c[s, pos], count_c[s, pos] = index[i, k], count[i, k]
        where[k] = (pos, act)
    tr_c, lc, ec, vc = _run_group(dev, inits, perm, index_c, count_c, seeds, dims)
    assert tuple(va.shape) == (S, G, B, C2)
    for k in range(G):
        tr_s, ls, es, vs = singles[k]
        pos, act = where[k]
        for i in range(S):
            n = int(count[i, k])
            for (l2, e2, v2, s2, gg) in ((ls, es, vs, i, 0), (lc, ec, vc, act[i], pos)):
                assert torch.equal(la[i, k], l2[s2, gg]), (k, i)
                assert torch.equal(ea[i, k, :n], e2[s2, gg, :n]) and torch.equal(va[i, k, :n], v2[s2, gg, :n]), (k, i)
        assert torch.isfinite(la[:, k]).all() and int(tr_a.step[k]) == S
        for x in ("flat", "flat_grad", "m", "v", "step"):
            a = getattr(tr_a, x)[k]
            assert torch.equal(a, getattr(tr_s, x)[0]) and torch.equal(a, getattr(tr_c, x)[pos]), (k, x)
    # dropout is on: the same model with another seed trains differently
    other = _run_group(dev, inits, [0], index[:, :1], count[:, :1], [s ^ 1 for s in seeds], dims)[0]
    assert not torch.equal(other.flat[0], tr_a.flat[0])
    # an idle step leaves a model's parameters, gradients, moments and counter alone while the others train
    before = {x: getattr(tr_c, x).clone() for x in ("flat", "flat_grad", "m", "v", "step")}
    cnt = np.full((1, G), B, dtype=np.int32)
    cnt[0, 1] = 0
    tr_c.run(index_c[:1], cnt, True)
    for x, b in before.items():
        assert torch.equal(getattr(tr_c, x)[1], b[1]), x
        assert not torch.equal(getattr(tr_c, x)[0], b[0]), x


def _np_mask(seed, step, site, rows, cols, p):
    """The documented hash of the mer_fusion_topn_group_* ABI (csrc/fusion_topn_group.hip, shift 27), restated in numpy: ctr = step << 32 | site << 27 | row << 16 | col."""
    with np.errstate(over="ignore"):
        r = np.arange(rows, dtype=np.uint64)[:, None]
        c = np.arange(cols, dtype=np.uint64)[None, :]
        ctr = (np.uint64(step & 0xFFFFFFFF) << np.uint64(32)) | (np.uint64(site) << np.uint64(27)) | (r << np.uint64(16)) | c
        z = np.uint64(seed) + (ctr + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).astype(np.uint8)


@pytest.mark.parametrize("M", [6, 18])
def test_topn_dropout_mask_is_the_documented_hash(dev, M):
    from mertools_amd.fusion_topn_group import dropout_mask
    for seed, step, p in ((0, 0, 0.3), (0xDEADBEEFCAFEF00D, 7, 0.5), (12345, 1 << 20, 0.2)):
        for site in (0, M - 1, M):
            got = dropout_mask(seed, step, site, 33, 300, p, dev).cpu().numpy()
            assert np.array_equal(got, _np_mask(seed, step, site, 33, 300, p)), (seed, step, site)
    got = dropout_mask(5, 2, M, 2048, 40, 0.3, dev).cpu().numpy()          # the largest row index, the widest site field
    assert np.array_equal(got, _np_mask(5, 2, M, 2048, 40, 0.3))
    big = dropout_mask(99, 3, M, 256, 512, 0.3, dev).float().mean().item()
    assert abs(big - 0.7) < 0.01, big
    base = dropout_mask(1, 2, 0, 32, 128, 0.4, dev)
    for other in (dropout_mask(2, 2, 0, 32, 128, 0.4, dev), dropout_mask(1, 3, 0, 32, 128, 0.4, dev), dropout_mask(1, 2, M, 32, 128, 0.4, dev)):
        assert not torch.equal(base, other)


def test_topn_dropout_training_matches_cpu_composition(dev):
    """3 train steps at p = 0.3 (M = 6, emotion head only) against a CPU composition of the oracle's pieces with the same masks
    (x * keep / (1 - p) at the six encoder inputs, sites 0..5, and the attention_mlp input, site 6): losses and parameters
    within 1e-4 (test_dropout_training_matches_cpu_composition's bound)."""
    import torch.nn.functional as F
    from oracle import fusion_ref as R
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer, dropout_mask
    p, B, S, seed, dims, H = 0.3, 16, 3, 0xABCDEF, DIMS6, 32
    M = len(dims)
    m = _models(dev, 1, 31, dims, dropout=p, H=H)[0]
    sd = {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items() if v.numel()}
    feats, emos, _ = _tables(64, dims, seed=4)
    tr = FusionTopnGroupTrainer([m], lr=1e-3, weight_decay=1e-5, grad_clip=-1.0, seeds=[seed], batch_size=B)
    tr.set_tables(feats, emos)
    index, count = _schedule(1, S, B, 64, 2, partial=[(0, 9)])
    loss = tr.run(index, count, True)[0].cpu().numpy()[:, 0]
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    ms = {k: torch.zeros_like(v) for k, v in sd.items()}
    vs = {k: torch.zeros_like(v) for k, v in sd.items()}
    for s in range(S):
        n = int(count[s, 0])
        rows = torch.as_tensor(index[s, 0, :n], dtype=torch.long)
        keeps = [dropout_mask(seed, s, site, n, w, p, dev).cpu().float() for site, w in enumerate(list(dims) + [M * H])]
        prm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        enc = [R.mlp_encoder(prm, f"encoder{i}", feats[i][rows] * keeps[i] * scale) for i in range(M)]
        mh = torch.cat(enc, dim=1)
        att = F.linear(R.mlp_encoder(prm, "attention_mlp", mh * keeps[M] * scale), prm["fc_att.weight"], prm["fc_att.bias"])
        fused = torch.matmul(torch.stack(enc, dim=2), att.unsqueeze(2)).squeeze(2)
        e = F.linear(fused, prm["fc_out_1.weight"], prm["fc_out_1.bias"])
        ref_loss = R.ce_loss(e, emos[rows])
        grads = torch.autograd.grad(ref_loss, list(prm.values()))
        with torch.no_grad():
            for (k, w), g in zip(list(prm.items()), grads):
                sd[k], ms[k], vs[k] = R.adam_step(w.detach(), g, ms[k], vs[k], s + 1, lr=1e-3, wd=1e-5)
        print(f"step {s}: loss {loss[s]:.7f} vs cpu {ref_loss.item():.7f}")
        assert abs(loss[s] - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item())), (s, loss[s], ref_loss.item())
    for k, w in m.model.state_dict().items():
        if w.numel():
            assert_close(w.cpu(), sd[k], 1e-4, f"dropout final {k}")


@pytest.mark.parametrize("dims,C2", [(DIMS6, 0), (DIMS18, 1)], ids=["M6", "M18"])
def test_topn_eval_step(dev, dims, C2):
    """An eval step leaves parameters, moments and step counters alone, and its emotion logits (and valence outputs) are
    torch.equal to the same module's own eval-mode forward through the single-model HIP ops (linear / FuseFn)."""
    from mertools_amd.fusion_topn_group import FusionTopnGroupTrainer
    G, B = 2, 16
    ms = [_models(dev, 1, 40 + k, dims, dropout=0.3, C2=C2)[0] for k in range(G)]
    feats, emos, vals = _tables(100, dims, seed=6)
    tr = FusionTopnGroupTrainer(ms, lr=1e-3, weight_decay=0.0, grad_clip=-1.0, batch_size=B)
    tr.set_tables(feats, emos, vals if C2 else None)
    index, count = _schedule(G, 2, B, 100, 7, partial=[(1, 3)])
    before = (tr.flat.clone(), tr.m.clone(), tr.v.clone(), tr.step.clone())
    loss, emo, val = (x.clone() for x in tr.run(index, count, False))
    for x, b in zip((tr.flat, tr.m, tr.v, tr.step), before):
        assert torch.equal(x, b)
    for k in range(G):
        ms[k].eval()
        for s in range(2):
            n = int(count[s, k])
            rows = torch.as_tensor(index[s, k, :n], dtype=torch.long)
            with torch.no_grad():
                _, e, v, _ = ms[k]({f"feat{i}": feats[i][rows].to(dev) for i in range(len(dims))})
            assert torch.equal(emo[s, k, :n], e), (k, s, (emo[s, k, :n] - e).abs().max().item())
            assert torch.equal(val[s, k, :n], v), (k, s)
            ce = torch.nn.functional.cross_entropy(e.double(), emos[rows].to(dev))
            mse = ((v.double().view(-1) - vals[rows].to(dev).double()) ** 2).mean() if C2 else 0.0
            assert abs(loss[s, k].item() - float(ce + mse)) < 1e-5 * max(1.0, float(ce + mse)), (k, s)


def _files(d):
    return sorted(f.rsplit("_", 1)[0] for f in os.listdir(d))


def _strip_scores(files):
    """result-file names up to the score and time-stamp parts: '<kind>_<prefix>_f1:..._acc:..._<time>.npz' -> '<kind>_<prefix>'."""
    return sorted(f.split("_f1:")[0] for f in files)


def _cli(tmp_path, dataset, dropout, batch=8):
    data = topn_corpus(tmp_path, dataset, n_train=50, n_test=9, dims=(24, 16, 20, 33, 12, 40))
    hyper = tmp_path / f"tune_{dropout}.yaml"
    hyper.write_text(f"attention_topn:\n  hidden_dim: 32\n  dropout: {dropout}\n  grad_clip: -1\n  lr: 1.0e-3\n")
    return base_argv(dataset) + ["--batch_size", str(batch), "--gpu", "0", "--data_root", str(data), "--hyper_path", str(hyper)]


@pytest.mark.parametrize("dataset", ["MER2024", "MER2026"])
def test_main_release_parallel_folds_against_default_path(dev, tmp_path, dataset):
    """--fusion_topn 2 --fusion_modality AVT, dropout 0, one epoch: --parallel_folds --seed s and the default path with --seed s write
    the same set of result files (up to score and time stamp), the same names order in every fold's eval and test store, and
    emotion outputs within 1e-4 of the default path's (which runs torch's CE and Adam, so not bitwise)."""
    from mertools_amd import main_release
    base = _cli(tmp_path, dataset, 0.0) + ["--epochs", "1", "--seed", "3"]
    res_d = main_release.main(base + ["--save_root", str(tmp_path / "seq")])
    res_p = main_release.main(base + ["--save_root", str(tmp_path / "par"), "--parallel_folds"])
    fd, fp = os.listdir(tmp_path / "seq-others-multitop" / "result"), os.listdir(tmp_path / "par-others-multitop" / "result")
    assert _strip_scores(fd) == _strip_scores(fp) and len(fd) == 2
    assert all(f"dataset:{dataset}_model:attention_topn" in f and "fusiontopn:2_modality:AVT" in f for f in fp)
    test_file = [f for f in fp if f.startswith("test1_")][0]
    assert np.load(tmp_path / "par-others-multitop" / "result" / test_file, allow_pickle=True)["emo_probs"].shape == (9, 6)
    assert len(res_d) == len(res_p) == 5
    worst = 0.0
    for f, (a, b) in enumerate(zip(res_d, res_p)):
        assert set(a) == set(b)
        for k in a:
            if k.endswith("_names"):
                assert a[k] == b[k], (f, k)
            elif k.endswith("_emolabels"):
                assert np.array_equal(a[k], b[k]), (f, k)
        for k in ("eval_emoprobs", "test1_emoprobs"):
            worst = max(worst, rel_err(torch.from_numpy(b[k]), torch.from_numpy(a[k]))[0])
    print(f"{dataset}: max-norm rel err of the grouped emotion outputs against the default path after one epoch: {worst:.3e}")
    for f, (a, b) in enumerate(zip(res_d, res_p)):
        for k in ("eval_emoprobs", "test1_emoprobs"):
            assert_close(torch.from_numpy(b[k]), torch.from_numpy(a[k]), 1e-4, f"{dataset} fold {f} {k} (worst over all: {worst:.3e})")


def _same_store(a_list, b_list):
    assert len(a_list) == len(b_list)
    for a, b in zip(a_list, b_list):
        assert set(a) == set(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k


def test_main_release_num_trials_equals_parallel_folds_runs(dev, tmp_path):
    """--num_trials 2 --seed s at dropout 0.3 writes, per trial, arrays np.array_equal to a --parallel_folds --seed s and a
    --parallel_folds --seed s+1 run (group invariance seen from the CLI: 10 models in one group against two groups of 5), and
    the same file names up to the time stamp."""
    from mertools_amd import main_release
    base = _cli(tmp_path, "MER2026", 0.3) + ["--epochs", "2"]
    res_t = main_release.main(base + ["--num_trials", "2", "--seed", "7", "--save_root", str(tmp_path / "trials")])
    assert len(res_t) == 2
    singles = []
    for t in range(2):
        res = main_release.main(base + ["--parallel_folds", "--seed", str(7 + t), "--save_root", str(tmp_path / "single")])
        _same_store(res, res_t[t])
        for fold in res:
            for k, x in fold.items():
                if isinstance(x, np.ndarray) and x.dtype.kind == "f":
                    assert np.isfinite(x).all(), k
        singles.append(res)
    assert not np.array_equal(singles[0][0]["eval_emoprobs"], singles[1][0]["eval_emoprobs"])
    got, want = _files(tmp_path / "trials-others-multitop" / "result"), _files(tmp_path / "single-others-multitop" / "result")
    assert got == want and len(got) == 4
