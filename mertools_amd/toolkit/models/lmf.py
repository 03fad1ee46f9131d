"""LMF (Low-rank Multimodal Fusion) — mirror of MERBench/toolkit/models/lmf.py:11-92 on the HIP kernels: the three
modality encoders, then the whole low-rank fusion (three [B,H+1] x [R,H+1,O] products, their element-wise product, the
rank-weighted sum and the bias) in one launch each way (fusion_ops.lmf_fuse -> mer_lmf_fwd / mer_lmf_bwd)."""
import torch
import torch.nn as nn
from torch.nn.init import xavier_normal_
from torch.nn.parameter import Parameter

from ...fusion_ops import linear, lmf_fuse
from .modules.encoder import LSTMEncoder, MLPEncoder


class LMF(nn.Module):
    def __init__(self, args):
        super().__init__()
        hidden_dim, rank, p = args.hidden_dim, args.rank, args.dropout
        self.grad_clip = args.grad_clip
        if args.feat_type not in ('utt', 'frm_align', 'frm_unalign'):
            raise ValueError(f"LMF: feat_type {args.feat_type!r}; 'utt', 'frm_align' or 'frm_unalign'")
        # construction order = the reference's (audio, text, video; factors; heads): the same torch.manual_seed gives the same initial values
        enc = MLPEncoder if args.feat_type == 'utt' else LSTMEncoder
        self.audio_encoder = enc(args.audio_dim, hidden_dim, p)
        self.text_encoder = enc(args.text_dim, hidden_dim, p)
        self.video_encoder = enc(args.video_dim, hidden_dim, p)
        self.output_dim = hidden_dim // 2
        self.post_fusion_dropout = nn.Dropout(p=p)   # defined and never applied by the reference; not applied here either
        self.audio_factor = Parameter(torch.empty(rank, hidden_dim + 1, self.output_dim))
        self.video_factor = Parameter(torch.empty(rank, hidden_dim + 1, self.output_dim))
        self.text_factor = Parameter(torch.empty(rank, hidden_dim + 1, self.output_dim))
        self.fusion_weights = Parameter(torch.empty(1, rank))
        self.fusion_bias = Parameter(torch.empty(1, self.output_dim))
        xavier_normal_(self.audio_factor)
        xavier_normal_(self.video_factor)
        xavier_normal_(self.text_factor)
        xavier_normal_(self.fusion_weights)
        self.fusion_bias.data.fill_(0)
        self.fc_out_1 = nn.Linear(self.output_dim, args.output_dim1)
        self.fc_out_2 = nn.Linear(self.output_dim, args.output_dim2)

    def forward(self, batch):
        audio_h = self.audio_encoder(batch['audios'])
        video_h = self.video_encoder(batch['videos'])
        text_h = self.text_encoder(batch['texts'])
        features = lmf_fuse(audio_h, video_h, text_h, self.audio_factor, self.video_factor, self.text_factor,
                            self.fusion_weights, self.fusion_bias)
        emos_out = linear(features, self.fc_out_1)
        vals_out = linear(features, self.fc_out_2)
        interloss = torch.zeros((), dtype=torch.int64, device=features.device)
        return features, emos_out, vals_out, interloss
