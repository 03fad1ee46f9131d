"""Grouped fusion training: G independent Attention models (the 5 folds of a cross-validation run times N hyper-parameter
trials) trained by ONE captured step of libmer_hip.so's mer_fusion_group_step (the 3-stream ABI of the group engine,
csrc/fusion_topn_group.hip).

The minibatches are gathered on the device from split tables uploaded once; an epoch is one [S, G, B] index table and one
[S, G] row-count table, walked by replaying the captured train / eval step S times (a device cursor the step advances picks
the slice, so no replay needs a host copy); outputs land in device epoch buffers that come back in one copy per epoch.
Every module's parameters are re-pointed at its row of the [G, P] buffer (as FusionGraphTrainer does), so state_dict()
reads the trained weights.  At dropout 0 a model's results are bitwise FusionGraphTrainer's on the same minibatches.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .ops import _p, stream


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def dropout_seed(seed, fold):
    """The dropout-mask seed of `fold` in a run with effective seed `seed` (main_release --parallel_folds)."""
    return _splitmix64(_splitmix64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ int(fold))


def dropout_mask(seed, step, site, rows, cols, p, device="cuda"):
    """uint8 [rows, cols] keep mask the group step uses at (seed, step, site) (mer_fusion_group_dropout_mask)."""
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().mer_fusion_group_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(site), rows, cols, float(p),
                                                        _p(keep), stream()), "mer_fusion_group_dropout_mask")
    return keep


def _attention_of(m):
    from .toolkit.models.attention import Attention
    net = getattr(m, "model", m)
    if not isinstance(net, Attention) or type(net.audio_encoder).__name__ != "MLPEncoder":
        raise _lib.MerError("FusionGroupTrainer supports the Attention model with feat_type 'utt' (MLPEncoders) only")
    if net.fc_out_1.out_features == 0 or net.fc_out_2.out_features != 1:
        raise _lib.MerError("FusionGroupTrainer supports the emotion + valence heads (MER2023) only")
    return net


class FusionGroupTrainer:
    """G models from toolkit.models.get_models (same Da, Dt, Dv, hidden_dim, both heads) with per-model lr, weight decay,
    grad clip (<= 0: none) and dropout seed.  Dropout p is read from each model's modules.

        tr = FusionGroupTrainer(models, lr=[...], weight_decay=[...], grad_clip=[...], seeds=[...], batch_size=32)
        tr.set_tables(audios, texts, videos, emos, vals)            # each split once, [N, D] float32 / [N] labels
        loss, emo, val = tr.run(index, count, train)                # index [S, G, B], count [S, G]; train: bool or [S] bools
    """

    # ---- what a group of another model states (fusion_topn_group.FusionTopnGroupTrainer), besides set_tables ----
    _ABI = "mer_fusion_group"   # the C entry points: <_ABI>_workspace_bytes and <_ABI>_step on the matching descriptor

    _net = staticmethod(_attention_of)   # the supported network inside a model, or MerError

    @staticmethod
    def _arch(n):
        return (n.audio_encoder.linear_1.in_features, n.text_encoder.linear_1.in_features, n.video_encoder.linear_1.in_features,
                n.fc_att.in_features, n.fc_out_1.out_features, n.fc_out_2.out_features)

    def _set_arch(self, arch):
        self.Da, self.Dt, self.Dv, self.H, self.C1, self.C2 = arch

    def _param_count(self):
        return _lib.lib().mer_fusion_group_param_count(self.Da, self.Dt, self.Dv, self.H, self.C1, self.C2)

    @staticmethod
    def _dropout_p(n):
        return n.audio_encoder.drop.p

    def _val_shape(self, S):
        return (S, self.G, self.B)

    def _new_desc(self):
        """The step descriptor, all but its workspace."""
        t = self._tables
        return _lib.FusionGroup(G=self.G, B=self.B, n_steps=self._cap, Da=self.Da, Dt=self.Dt, Dv=self.Dv, H=self.H, C1=self.C1,
                                C2=self.C2, feat_a=_p(t["a"]), feat_t=_p(t["t"]), feat_v=_p(t["v"]), emo=_p(t["emo"]), val=_p(t["val"]),
                                out_val=_p(self.out_val), **self._common_fields())

    # ---- the common part ----
    def __init__(self, models, lr, weight_decay, grad_clip, seeds=None, batch_size=32):
        name = type(self).__name__
        G = len(models)
        if G == 0:
            raise _lib.MerError(f"{name} needs at least one model")
        nets = [self._net(m) for m in models]
        arch = self._arch(nets[0])
        for n in nets:
            if self._arch(n) != arch:
                raise _lib.MerError(f"a group holds models of one architecture: {self._arch(n)} != {arch}")
        self._set_arch(arch)
        self.G, self.B = G, int(batch_size)
        self.models = models
        P = self._param_count()
        params0 = [p for p in models[0].parameters() if p.requires_grad]
        if not params0[0].is_cuda:
            raise _lib.MerError(f"{name} needs the models on the GPU (there is no CPU path)")
        dev = params0[0].device
        if sum(p.numel() for p in params0) != P:
            raise _lib.MerError("parameter count differs from the grouped kernels' layout")
        self.P, self.dev = P, dev
        self.flat = torch.empty((G, P), dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros((G, P), dtype=torch.float32, device=dev)
        self.m = torch.zeros((G, P), dtype=torch.float32, device=dev)
        self.v = torch.zeros((G, P), dtype=torch.float32, device=dev)
        self.step = torch.zeros(G, dtype=torch.int32, device=dev)
        for g, mdl in enumerate(models):   # re-point every parameter (and its .grad) at row g of the group buffers
            off = 0
            for p in (q for q in mdl.parameters() if q.requires_grad):
                k = p.numel()
                self.flat[g, off:off + k].copy_(p.data.reshape(-1))
                p.data = self.flat[g, off:off + k].view_as(p.data)
                p.grad = self.flat_grad[g, off:off + k].view_as(p.data)
                off += k

        def per_model(x, name):
            x = list(x) if isinstance(x, (list, tuple, np.ndarray)) else [x] * G
            if len(x) != G:
                raise _lib.MerError(f"{name}: {len(x)} values for {G} models")
            return x

        self.lr = torch.tensor(per_model(lr, "lr"), dtype=torch.float32, device=dev)
        self.wd = torch.tensor(per_model(weight_decay, "weight_decay"), dtype=torch.float32, device=dev)
        self.clip = torch.tensor([float(c) for c in per_model(grad_clip, "grad_clip")], dtype=torch.float32, device=dev)
        self.dropout = torch.tensor([float(self._dropout_p(n)) for n in nets], dtype=torch.float32, device=dev)
        seeds = per_model(seeds if seeds is not None else 0, "seeds")   # uint64 bits carried in an int64 tensor
        self.seed = torch.from_numpy(np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], dtype=np.uint64).view(np.int64)).to(dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self._tables = None
        self._cap = 0
        self._graphs = {}
        self._ws = None   # sized by (architecture, G, B), which a trainer never changes: allocated once

    # ---- data ----
    def set_tables(self, audios, texts, videos, emos, vals):
        """Upload one split table (host or device): [N, Da] / [N, Dt] / [N, Dv] float32, emos [N] class ids, vals [N]."""
        def f32(x):
            return torch.as_tensor(x).to(self.dev, torch.float32).contiguous()
        t = dict(a=f32(audios), t=f32(texts), v=f32(videos), emo=torch.as_tensor(emos).to(self.dev, torch.int32).contiguous(),
                 val=f32(vals).reshape(-1))
        n = t["a"].shape[0]
        if (t["a"].shape[1], t["t"].shape[1], t["v"].shape[1]) != (self.Da, self.Dt, self.Dv) or any(t[k].shape[0] != n for k in t):
            raise _lib.MerError("split tables: shapes do not match the models' input dims / each other")
        self._tables = t
        self._graphs = {}

    def _reserve(self, S):
        if S <= self._cap:
            return
        G, B, dev = self.G, self.B, self.dev
        self._cap = S
        self.index = torch.zeros((S, G, B), dtype=torch.int32, device=dev)
        self.count = torch.zeros((S, G), dtype=torch.int32, device=dev)
        self.out_loss = torch.zeros((S, G), dtype=torch.float32, device=dev)
        self.out_emo = torch.zeros((S, G, B, self.C1), dtype=torch.float32, device=dev)
        self.out_val = torch.zeros(self._val_shape(S), dtype=torch.float32, device=dev)
        self._graphs = {}

    def _common_fields(self):
        """The descriptor fields both ABIs spell alike."""
        return dict(P=self.P, params=_p(self.flat), grads=_p(self.flat_grad), adam_m=_p(self.m), adam_v=_p(self.v),
                    step=_p(self.step), lr=_p(self.lr), weight_decay=_p(self.wd), grad_clip=_p(self.clip),
                    dropout=_p(self.dropout), seed=_p(self.seed), beta1=0.9, beta2=0.999, eps=1e-8,
                    n_rows=self._tables["a"].shape[0], index=_p(self.index), count=_p(self.count), cursor=_p(self.cursor),
                    out_loss=_p(self.out_loss), out_emo=_p(self.out_emo))

    def _desc(self):
        d = self._new_desc()
        if self._ws is None:
            nbytes = getattr(_lib.lib(), self._ABI + "_workspace_bytes")(ctypes.byref(d))
            if nbytes < 0:
                _lib.check(int(nbytes), self._ABI + "_workspace_bytes")
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        d.workspace, d.workspace_bytes = _p(self._ws), self._ws.numel()
        return d

    def _launch(self, d, train):
        _lib.check(getattr(_lib.lib(), self._ABI + "_step")(ctypes.byref(d), int(train), stream()), self._ABI + "_step")

    def _graph(self, train):
        if train not in self._graphs:
            d = self._desc()
            # first launches outside the capture (module load); with every count 0 the step only advances the cursor
            saved = self.count[0].clone()
            self.count[0].zero_()
            self.cursor.zero_()
            self._launch(d, train)
            self.count[0].copy_(saved)
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch(d, train)
            self._graphs[train] = (g, d)
        return self._graphs[train][0]

    # ---- steps ----
    def run(self, index, count, train):
        """Walks S steps: index [S, G, B] rows of the split table, count [S, G] rows used (0 = idle); train: one bool for all
        steps or one per step.  Returns device (loss [S, G], emo logits [S, G, B, C1], valence [S, G, B]) — views of the
        epoch buffers, valid until the next run()."""
        if self._tables is None:
            raise _lib.MerError("FusionGroupTrainer.run: set_tables() first")
        index = torch.as_tensor(index, dtype=torch.int32)
        count = torch.as_tensor(count, dtype=torch.int32)
        S = index.shape[0]
        if tuple(index.shape) != (S, self.G, self.B) or tuple(count.shape) != (S, self.G):
            raise _lib.MerError(f"run: index {tuple(index.shape)} / count {tuple(count.shape)}, want [S, {self.G}, {self.B}] / [S, {self.G}]")
        n = self._tables["a"].shape[0]
        if int(count.min()) < 0 or int(count.max()) > self.B:
            raise _lib.MerError("run: row counts must lie in [0, batch_size]")
        used = torch.arange(self.B).view(1, 1, -1) < count.unsqueeze(-1).long()
        if bool(((index < 0) | (index >= n))[used].any()):
            raise _lib.MerError("run: index outside the split table")
        modes = [bool(train)] * S if isinstance(train, (bool, int)) else [bool(x) for x in train]
        if len(modes) != S:
            raise _lib.MerError("run: one train flag per step")
        self._reserve(S)
        graphs = {mode: self._graph(mode) for mode in set(modes)}
        self.index[:S].copy_(index)
        self.count.zero_()
        self.count[:S].copy_(count)
        self.cursor.zero_()
        for mode in modes:
            graphs[mode].replay()
        return self.out_loss[:S], self.out_emo[:S], self.out_val[:S]

    def train_step(self, index, count):
        """One train step on rows index [G, B] (count [G]); returns (loss [G], emo [G, B, C1], valence [G, B]) device views."""
        l, e, v = self.run(torch.as_tensor(index).view(1, self.G, self.B), torch.as_tensor(count).view(1, self.G), True)
        return l[0], e[0], v[0]

    def eval_step(self, index, count):
        l, e, v = self.run(torch.as_tensor(index).view(1, self.G, self.B), torch.as_tensor(count).view(1, self.G), False)
        return l[0], e[0], v[0]
