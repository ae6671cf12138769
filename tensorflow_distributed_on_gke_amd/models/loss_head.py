"""The loss head of Transformer.loss_and_backward: vocabulary projection,
masked cross entropy / accuracy (or the distillation mixture), the final
layer's gradients and the gradient of the decoder output.

Two functions, one per device: gpu_head sequences the HIP kernels, cpu_head is
the f32 PyTorch definition the CPU tests hold them to. Each writes `step_out`
([loss / workers, accuracy]), adds its record to `accum` ([sum loss, sum acc,
n, n labels]) and, under distillation, the label cross entropy's to
`label_accum`; writes the final layer's gradients (adds to them with
rt.accumulate); and returns the gradient of `dec` as [B*T, d_model], or None
without `backward`.

The loss divisor is resolved once per head: the batch's own label count,
unless `ntok_total` (the count of a whole accumulated update) replaces it or
the `ntok_sum` all-reduce turns it into the count over all replicas.
"""
from __future__ import annotations

import torch

from tensorflow_distributed_on_gke_amd.models.layers import _dgrad_res, _wgrad
from tensorflow_distributed_on_gke_amd.ops import kernels as K

PAD_ID = 0


def gpu_head(model, rt, dec, labels, ntok, ntok_work, ntok_total, workers, step_out, accum,
             label_accum, backward, t_logits, teacher, alpha):
    """ntok: this batch's label count from prep_batch; ntok_work: the handle
    of its all-reduce, started before the forward (or None); t_logits: the
    teacher's logits (None: no distillation)."""
    cfg = model.cfg
    dev = dec.device
    M = labels.numel()
    dec2 = dec.detach().reshape(M, cfg.d_model)
    logits = model.project(dec.detach())
    row_loss = K.workspace("row_loss", M, dev)[:M]
    row_cor = K.workspace("row_correct", M, dev)[:M]
    # the divisor (the wait stays here, after the projection's launch: the
    # all-reduce has had the whole forward to finish)
    if ntok_total is not None:
        ntok = ntok_total
    if ntok_work is not None:
        ntok_work.wait()
    if t_logits is not None:
        row_lab = K.workspace("row_label", M, dev)[:M]
        K.xent_distill(logits, t_logits, cfg.tgt_vocab, labels, ntok, workers,
                       cfg.label_smoothing, alpha, teacher.weights, row_loss, row_cor,
                       row_lab, write_grad=backward)
        if label_accum is not None:
            K.xent_stats(row_lab, row_cor, ntok, workers, None, label_accum)
    else:
        K.xent(logits, cfg.tgt_vocab, labels, ntok, workers, cfg.label_smoothing, row_loss,
               row_cor, write_grad=backward)
    K.xent_stats(row_loss, row_cor, ntok, workers, step_out, accum)
    if not backward:
        return None
    dl = logits  # now holds dlogits (pad columns zeroed)
    _wgrad(rt, dl, dec2.contiguous(), cfg.tgt_vocab, model.final.w, model.final.b)
    return _dgrad_res(dl, model.final.w, cfg.tgt_vocab, None)


def cpu_head(model, rt, dec, labels, ntok_sum, ntok_total, workers, step_out, accum,
             label_accum, backward, t_logits, teacher, alpha):
    """ntok_sum: called with this replica's label count, turns it in place
    into the count over all replicas (or None); t_logits: the teacher's
    logits (None: no distillation)."""
    cfg = model.cfg
    dec2 = dec.detach().reshape(labels.numel(), cfg.d_model)
    lg = model.project(dec.detach())
    lab = labels.reshape(-1)
    mask = (lab != PAD_ID).to(torch.float32)
    # the divisor
    ntok = mask.sum() if ntok_total is None else ntok_total.reshape(()).clone()
    if ntok_sum is not None:
        w = ntok_sum(ntok)
        if w is not None:
            w.wait()
    ntok = ntok.clamp_min(1.0)
    logp = torch.log_softmax(lg, dim=-1)
    eps = cfg.label_smoothing
    nll = -logp.gather(1, lab.view(-1, 1)).squeeze(1)
    smooth = -logp.mean(dim=-1)
    row_loss = ((1 - eps) * nll + eps * smooth) * mask
    correct = ((lg.argmax(dim=-1) == lab).to(torch.float32) * mask).sum()
    acc = correct / ntok
    if t_logits is not None:
        if label_accum is not None:
            label_loss = row_loss.sum() / ntok / workers
            label_accum += torch.stack([label_loss, acc, torch.tensor(1.0), ntok])
        target = K.distill_target(t_logits, cfg.tgt_vocab, lab, eps, alpha, teacher.weights)
        row_loss = -(target * logp).sum(dim=-1) * mask
    loss = row_loss.sum() / ntok / workers
    step_out.copy_(torch.stack([loss, acc]).detach())
    if accum is not None:
        accum += torch.stack([loss.detach(), acc.detach(), torch.tensor(1.0), ntok])
    if not backward:
        return None
    if t_logits is not None:
        dl = torch.softmax(lg, -1) - target
    else:
        onehot = torch.nn.functional.one_hot(lab, cfg.tgt_vocab).to(torch.float32)
        dl = (torch.softmax(lg, -1) - (1 - eps) * onehot - eps / cfg.tgt_vocab)
    dl = dl * (mask / (ntok * workers)).view(-1, 1)
    fw, fb = model.final.w, model.final.b
    g_w = dl.t() @ dec2
    g_b = dl.sum(0)
    if rt.accumulate:
        fw.grad.add_(g_w)
        fb.grad.add_(g_b)
    else:
        fw.grad.copy_(g_w)
        fb.grad.copy_(g_b)
    if rt.store is not None:
        rt.store.grad_ready(fw)
        rt.store.grad_ready(fb)
    return dl @ fw.master
