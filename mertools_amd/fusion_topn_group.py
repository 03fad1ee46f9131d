"""Grouped Attention_TOPN training: G independent Attention_TOPN models (the 5 folds of a cross-validation run times N
hyper-parameter trials of the MER2024 / MER2025 / MER2026 multi-feature recipe) trained by ONE captured step of libmer_hip.so's
mer_fusion_topn_group_step (csrc/fusion_topn_group.hip).

The surface is fusion_group.FusionGroupTrainer's: split tables uploaded once (here a list of M feature tables), an epoch as one
[S, G, B] index table and one [S, G] row-count table walked by replaying the captured train / eval step through a device cursor,
outputs in device epoch buffers, every module's parameters re-pointed at its row of the [G, P] buffer so state_dict() reads the
trained weights.  The valence head may be absent (output_dim2 = 0, the MER2024-2026 corpora): the loss is then CE alone and the
valence output is an empty [S, G, B, 0] tensor.
"""
import ctypes

import torch

from . import _lib
from .fusion_group import FusionGroupTrainer, dropout_seed  # noqa: F401  (the same (effective seed, fold) -> mask seed rule)
from .ops import _p, stream

MAX_STREAMS = 18


def dropout_mask(seed, step, site, rows, cols, p, device="cuda"):
    """uint8 [rows, cols] keep mask the grouped Attention_TOPN step uses at (seed, step, site): site i < M is the input of
    encoder i, site M the input of attention_mlp (mer_fusion_topn_group_dropout_mask)."""
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().mer_fusion_topn_group_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(site), rows, cols, float(p),
                                                             _p(keep), stream()), "mer_fusion_topn_group_dropout_mask")
    return keep


def param_count(feat_dims, H, C1, C2):
    """Parameters of one Attention_TOPN model as the grouped kernels lay them out (raises MerError on an unsupported shape)."""
    dims = (ctypes.c_int * len(feat_dims))(*[int(d) for d in feat_dims])
    P = _lib.lib().mer_fusion_topn_group_param_count(len(feat_dims), dims, int(H), int(C1), int(C2))
    if P < 0:
        _lib.check(int(P), "mer_fusion_topn_group_param_count")
    return int(P)


def _topn_of(m):
    from .toolkit.models.attention_topn import Attention_TOPN
    net = getattr(m, "model", m)
    if not isinstance(net, Attention_TOPN):
        raise _lib.MerError("FusionTopnGroupTrainer supports the Attention_TOPN model (feat_type 'utt') only")
    return net


def _arch(net):
    return (tuple(int(d) for d in net.feat_dims), net.fc_att.in_features, net.fc_out_1.out_features, net.fc_out_2.out_features)


class FusionTopnGroupTrainer(FusionGroupTrainer):
    """G models from toolkit.models.get_models (Attention_TOPN, one (feat_dims, hidden_dim, C1, C2)) with per-model lr, weight
    decay, grad clip (<= 0: none) and dropout seed.  Dropout p is read from each model's modules.

        tr = FusionTopnGroupTrainer(models, lr=[...], weight_decay=[...], grad_clip=[...], seeds=[...], batch_size=32)
        tr.set_tables(feats, emos, vals)             # feats: M tables [N, D_i] float32; emos [N]; vals [N] (None when C2 = 0)
        loss, emo, val = tr.run(index, count, train)                # index [S, G, B], count [S, G]; train: bool or [S] bools

    run / train_step / eval_step and the captured graphs are FusionGroupTrainer's; the valence output is [S, G, B, C2].
    """

    _ABI = "mer_fusion_topn_group"
    _net = staticmethod(_topn_of)
    _arch = staticmethod(_arch)

    def _set_arch(self, arch):
        self.D, self.H, self.C1, self.C2 = arch
        self.M = len(self.D)

    def _param_count(self):
        return param_count(self.D, self.H, self.C1, self.C2)

    @staticmethod
    def _dropout_p(n):
        return n.encoder0.drop.p

    def _val_shape(self, S):
        return (S, self.G, self.B, self.C2)

    def _new_desc(self):
        t = self._tables
        d = _lib.FusionTopnGroup(G=self.G, B=self.B, n_steps=self._cap, M=self.M, H=self.H, C1=self.C1, C2=self.C2, emo=_p(t["emo"]),
                                 val=_p(t["val"]) if self.C2 else None, out_val=_p(self.out_val) if self.C2 else None,
                                 **self._common_fields())
        for i in range(self.M):
            d.D[i] = self.D[i]
            d.feat[i] = _p(t["feats"][i])
        return d

    # ---- data ----
    def set_tables(self, feats, emos, vals=None):
        """Upload one split table (host or device): M tables [N, D_i] float32, emos [N] class ids, vals [N] (needed when C2 = 1)."""
        def f32(x):
            return torch.as_tensor(x).to(self.dev, torch.float32).contiguous()
        feats = [f32(x) for x in feats]
        if len(feats) != self.M:
            raise _lib.MerError(f"split tables: {len(feats)} feature tables for {self.M} streams")
        emo = torch.as_tensor(emos).to(self.dev, torch.int32).contiguous()
        if self.C2 != 0 and vals is None:
            raise _lib.MerError("split tables: the valence head needs vals")
        val = f32(vals).reshape(-1) if vals is not None else None
        n = feats[0].shape[0]
        if (any(x.dim() != 2 or x.shape != (n, d) for x, d in zip(feats, self.D)) or emo.shape != (n,)
                or (val is not None and val.shape != (n,))):
            raise _lib.MerError("split tables: shapes do not match the models' input dims / each other")
        self._tables = dict(a=feats[0], feats=feats, emo=emo, val=val)   # "a": the table run() takes the row count from
        self._graphs = {}
