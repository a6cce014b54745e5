"""The masked-region objective as include/visualbert_hip.h states it for vb_visual_loss_fwd_bwd, in plain PyTorch on the CPU -- the
yardstick of tests/test_visual_loss.py.  It restates the loss lines of LXRTPretraining.forward
(unsupervised_visualbert/src/lxrt/modeling.py:1391-1420):

    loss_fcts = {'l2': SmoothL1Loss(reduction='none'), 'ce': CrossEntropyLoss(ignore_index=-1, reduction='none')}     :1392-1396
    visn_loss = visn_loss_fct(scores.view(-1, output_dim), label.view(*label_shape))                                 :1411-1414
    if visn_loss.dim() > 1: visn_loss = visn_loss.mean(1)                                                            :1415-1416
    visn_loss = (visn_loss * mask_conf.view(-1)).mean() * weight                                                     :1417

with the two torch calls the reference itself makes, and takes the gradient of the sum of the three terms by autograd.  Run twice:
in fp64 (the reference) and in fp32 (its distance from the fp64 run sizes the tolerance: what fp32 arithmetic costs on these very
numbers, whatever the order of the sums).  One deliberate addition, stated in the header: a class label outside [0, n) is ignored
like -1 (torch would raise)."""
import torch
import torch.nn.functional as F


def loss_terms(x, n_obj, n_attr, n_feat, obj_label, obj_conf, attr_label, attr_conf, feat_target, feat_conf, w_obj, w_attr, w_feat):
    """x: [M, n_obj + n_attr + n_feat] of the dtype to compute in (differentiable).  Returns [obj, attr, feat, sum] (0-d tensors)."""
    dtype = x.dtype
    zero = torch.zeros((), dtype=dtype)
    terms = []
    for off, n, label, conf, w in ((0, n_obj, obj_label, obj_conf, w_obj), (n_obj, n_attr, attr_label, attr_conf, w_attr)):
        if n == 0:
            terms.append(zero)
            continue
        lab = label.detach().cpu().reshape(-1).long()
        lab = torch.where((lab >= 0) & (lab < n), lab, torch.full_like(lab, -1))
        l = F.cross_entropy(x[:, off:off + n], lab, ignore_index=-1, reduction="none")
        terms.append((l * conf.detach().cpu().reshape(-1).to(dtype)).mean() * torch.tensor(w, dtype=dtype))
    if n_feat:
        off = n_obj + n_attr
        l = F.smooth_l1_loss(x[:, off:off + n_feat], feat_target.detach().cpu().reshape(-1, n_feat).to(dtype), reduction="none")
        l = l.mean(1)
        terms.append((l * feat_conf.detach().cpu().reshape(-1).to(dtype)).mean() * torch.tensor(w_feat, dtype=dtype))
    else:
        terms.append(zero)
    return terms + [terms[0] + terms[1] + terms[2]]


def visual_losses(scores, n_obj, n_attr, n_feat, *rest, dtype=torch.float64):
    """scores: [M, >= n_obj + n_attr + n_feat] (any float dtype; converted to `dtype` exactly); rest: the remaining arguments of
    loss_terms.  Returns (losses [4] = obj, attr, feat, sum; dscores [M, n_obj + n_attr + n_feat] = d losses[3] / d scores)."""
    width = n_obj + n_attr + n_feat
    x = scores.detach().cpu()[:, :width].to(dtype).clone().requires_grad_(True)
    terms = loss_terms(x, n_obj, n_attr, n_feat, *rest)
    grad = torch.zeros_like(x)
    if terms[3].requires_grad:
        grad, = torch.autograd.grad(terms[3], x)
    return torch.stack([t.detach() for t in terms]), grad.detach()


def bounds(r32, r64, floor=1e-7):
    """4 x the fp32 restatement's own distance from the fp64 one: (relative bound per loss [4], max-abs bound on the gradient with
    the absolute floor)"""
    (l32, g32), (l64, g64) = r32, r64
    rel = 4.0 * (l32.double() - l64).abs() / l64.abs().clamp_min(1e-300)
    return rel, max(4.0 * float((g32.double() - g64).abs().max()), floor)
