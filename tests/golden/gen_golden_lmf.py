#!/usr/bin/env python3
"""Generates tests/golden/fusion_lmf.npz by RUNNING THE REFERENCE'S OWN toolkit.models.lmf.LMF on the CPU (see gen_golden.py:
the module is imported from the reference tree at generation time, nothing of it is copied).

  * utt (no key prefix): audio 48 / text 40 / video 32 -> hidden 32, rank 4, heads 6 + 1, dropout 0, built under
    torch.manual_seed(1237).  init_*, the inputs x_* [5, 32, D], emos, vals, an eval forward of step 0's minibatch (out_*),
    then 5 steps of the reference's CELoss + MSELoss with Adam(lr 1e-3, weight decay 1e-5) exactly as
    gen_golden.fusion_goldens does them: losses, grad0_* (first-step gradients), final_*.
  * frm_align (prefix frm_): the same dims with three LSTMEncoders, T = 6, B = 8, torch.manual_seed(4321): init, inputs,
    forward outputs and first-step gradients.
  * f64diff_* / frm_f64diff_*: the same forward outputs and first-step gradients from a float64 copy of the reference model on
    the float64 inputs — how far the fp32 reference itself sits from the exact values.  The twin's float64 values themselves
    would put the file over the size of fusion_attention.npz (1013 KB against 821 KB), so what is stored is the float32
    DIFFERENCE twin - fp32, and the key says so (f64diff_X belongs to X): X.astype(float64) + f64diff_X restores the twin's
    value to ~1e-14 of its size, far below the ~1e-7 distances it is there to measure.

    python tests/golden/gen_golden_lmf.py
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, ref_toolkit  # noqa: E402

DIMS = dict(audio_dim=48, text_dim=40, video_dim=32, hidden_dim=32, rank=4, output_dim1=6, output_dim2=1, dropout=0.0, grad_clip=-1.0)


def _step0(model, batch, emos, vals, cls_loss, reg_loss):
    """Train-mode forward + backward of one minibatch: (outputs, gradients by parameter name, loss)."""
    model.zero_grad()
    f, e, v, il = model(batch)
    loss = il + cls_loss(e, emos) + reg_loss(v, vals)
    loss.backward()
    outs = dict(features=f.detach().numpy().copy(), emos_out=e.detach().numpy().copy(), vals_out=v.detach().numpy().copy())
    return outs, {k: p.grad.clone().numpy() for k, p in model.named_parameters()}, loss


def _twin64(model, batch, emos, vals, cls_loss, reg_loss):
    twin = copy.deepcopy(model).double().train()
    outs, grads, _ = _step0(twin, {k: x.double() for k, x in batch.items()}, emos, vals.double(), cls_loss, reg_loss)
    return outs, grads


def _diff(v64, v32):
    assert v64.dtype == np.float64 and v32.dtype == np.float32 and v64.shape == v32.shape
    return (v64 - v32.astype(np.float64)).astype(np.float32)


def lmf_goldens():
    ref_toolkit()
    from toolkit.models.lmf import LMF
    from toolkit.utils.loss import CELoss, MSELoss
    cls_loss, reg_loss = CELoss(), MSELoss()
    res = {}

    # ---- utterance level
    args = argparse.Namespace(feat_type="utt", **DIMS)
    torch.manual_seed(1237)
    model = LMF(args)
    res.update({f"init_{k}": v.clone().numpy() for k, v in model.state_dict().items()})
    B, steps = 32, 5
    xs = dict(audios=torch.randn(steps, B, 48), texts=torch.randn(steps, B, 40), videos=torch.randn(steps, B, 32))
    emos = torch.randint(0, 6, (steps, B))
    vals = torch.randn(steps, B) * 2
    batch0 = {k: x[0] for k, x in xs.items()}
    model.eval()
    with torch.no_grad():
        f, e, v, il = model(batch0)
    res.update(out_features=f.numpy().copy(), out_emos_out=e.numpy().copy(), out_vals_out=v.numpy().copy())
    o64, g64 = _twin64(model, batch0, emos[0], vals[0], cls_loss, reg_loss)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    losses = []
    for s in range(steps):
        opt.zero_grad()
        f, e, v, il = model({k: x[s] for k, x in xs.items()})
        loss = il + cls_loss(e, emos[s]) + reg_loss(v, vals[s])
        loss.backward()
        if s == 0:
            res.update({f"grad0_{k}": p.grad.clone().numpy() for k, p in model.named_parameters()})
        opt.step()
        losses.append(loss.item())
    res.update({f"final_{k}": v.clone().numpy() for k, v in model.state_dict().items()})
    res.update({f"f64diff_out_{k}": _diff(v, res[f"out_{k}"]) for k, v in o64.items()})
    res.update({f"f64diff_grad0_{k}": _diff(v, res[f"grad0_{k}"]) for k, v in g64.items()})
    res.update(losses=np.array(losses, dtype=np.float64), emos=emos.numpy(), vals=vals.numpy(), **{f"x_{k}": v.numpy() for k, v in xs.items()})
    print("utt losses", losses)

    # ---- frame level (LSTMEncoder x3)
    args = argparse.Namespace(feat_type="frm_align", **DIMS)
    torch.manual_seed(4321)
    model = LMF(args).train()
    res.update({f"frm_init_{k}": v.clone().numpy() for k, v in model.state_dict().items()})
    B, T = 8, 6
    batch = dict(audios=torch.randn(B, T, 48), texts=torch.randn(B, T, 40), videos=torch.randn(B, T, 32))
    emos, vals = torch.randint(0, 6, (B,)), torch.randn(B) * 2
    o64, g64 = _twin64(model, batch, emos, vals, cls_loss, reg_loss)
    outs, grads, loss = _step0(model, batch, emos, vals, cls_loss, reg_loss)
    res.update({f"frm_out_{k}": v for k, v in outs.items()})
    res.update({f"frm_grad0_{k}": v for k, v in grads.items()})
    res.update({f"frm_f64diff_out_{k}": _diff(v, outs[k]) for k, v in o64.items()})
    res.update({f"frm_f64diff_grad0_{k}": _diff(v, grads[k]) for k, v in g64.items()})
    res.update(frm_loss=np.array(loss.item()), frm_emos=emos.numpy(), frm_vals=vals.numpy(), **{f"frm_x_{k}": v.numpy() for k, v in batch.items()})
    print("frm_align loss", loss.item())

    path = os.path.join(OUT, "fusion_lmf.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes;", os.path.getsize(os.path.join(OUT, "fusion_attention.npz")), "for fusion_attention.npz")


if __name__ == "__main__":
    lmf_goldens()
