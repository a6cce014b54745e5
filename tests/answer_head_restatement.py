"""The answer head of the sibling LXRT model and its two losses in plain PyTorch on the CPU -- the yardstick of
tests/test_answer_head.py.  It restates, with the calls the reference itself makes,

    gelu(x) = x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))                                  lxrt/modeling.py:112-131 (GeLU)
    BertLayerNorm = torch.nn.LayerNorm                                                         lxrt/modeling.py:280
    logit_fc = Sequential(Linear(H, 2H), GeLU(), BertLayerNorm(2H, eps=1e-12), Linear(2H, A))  lxrt/modeling.py:956-969,
                                                                                               tasks/vqa_model.py:28-34
    loss = BCEWithLogitsLoss()(logit, target) * logit.size(1)                                  tasks/vqa.py:72, :106-107
    score, label = logit.max(1); the soft score of that label                                  tasks/vqa.py:114-117
    answer_loss = CrossEntropyLoss(ignore_index=-1)(answer_score.view(-1, A), ans.view(-1))    lxrt/modeling.py:1369, :1423-1427

and takes every gradient by autograd.  Each case runs twice: in fp64 (the reference) and in fp32 (its distance from the fp64 run
sizes the tolerance: what fp32 arithmetic costs on these very numbers, whatever the order of the sums).  The input builders of the
kernel tests live here too, so that the CPU suite can check the conditions they promise."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-12


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bert_layer_norm(x, weight, bias, eps=EPS):
    """the sibling's BertLayerNorm IS torch.nn.LayerNorm (lxrt/modeling.py:280): biased variance, eps inside the sqrt"""
    return F.layer_norm(x, (x.size(-1),), weight, bias, eps)


def layer_norm_written_out(x, weight, bias, eps=EPS):
    """the same thing spelled out (the other BERT port's BertLayerNorm.forward); tests/test_answer_head_host.py holds the two together"""
    u = x.mean(-1, keepdim=True)
    s = (x - u).pow(2).mean(-1, keepdim=True)
    return weight * ((x - u) / torch.sqrt(s + eps)) + bias


def ln_case(x, dy, gamma, beta, act, dtype, eps=EPS):
    """y = LN(act ? gelu(x) : x) and the gradients of sum(y * dy): dict(y, dx, dgamma, dbeta), computed in `dtype`"""
    xs = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    g = gamma.detach().cpu().to(dtype).clone().requires_grad_(True)
    b = beta.detach().cpu().to(dtype).clone().requires_grad_(True)
    y = bert_layer_norm(gelu(xs) if act else xs, g, b, eps)
    dx, dg, db = torch.autograd.grad(y, (xs, g, b), dy.detach().cpu().to(dtype))
    return dict(y=y.detach(), dx=dx, dgamma=dg, dbeta=db)


def bce_case(logits, target, dtype):
    """(loss, dlogits, score) of the VQA fine-tuning lines, computed in `dtype`"""
    x = logits.detach().cpu().to(dtype).clone().requires_grad_(True)
    t = target.detach().cpu().to(dtype)
    loss = torch.nn.BCEWithLogitsLoss()(x, t) * x.size(1)
    grad, = torch.autograd.grad(loss, x)
    _, label = x.detach().max(1)
    score = t[torch.arange(x.size(0)), label].mean()
    return loss.detach(), grad, score


def bound(a32, a64, floor=1e-7):
    """4 x the fp32 restatement's own max-abs distance from the fp64 one, with the floor floor * max|reference|"""
    return max(4.0 * float((a32.double() - a64).abs().max()), floor * float(a64.abs().max()))


def loss_rel_bound(l32, l64, M, V):
    """relative bound of the BCE loss: 4 x the fp32 restatement's relative distance, or what a pairwise sum of the M * V positive
    terms can lose in fp32, 2^-23 * ceil(log2(M V)), whichever is larger (the restatement's loss can land on the fp64 one by luck)"""
    rel = abs(float(l32) - float(l64)) / abs(float(l64))
    return max(4.0 * rel, 2.0 ** -23 * math.ceil(math.log2(M * V)))


# ---- input builders -------------------------------------------------------------------------------------------------------------
def ln_inputs(M, H, seed=0):
    """x ~ 1.5 N(0, 1) with a few entries at +-6 (erf saturated), gamma / beta away from their initial (1, 0), dy ~ N(0, 1)"""
    g = torch.Generator().manual_seed(100003 * seed + 31 * M + H)
    x = torch.randn((M, H), generator=g) * 1.5
    x[0, 0], x[0, H - 1], x[M - 1, H // 2], x[M // 2, 3] = 6.0, -6.0, 6.0, -6.0
    gamma = 0.5 + torch.rand(H, generator=g)
    beta = torch.randn(H, generator=g) * 0.5
    dy = torch.randn((M, H), generator=g)
    return x, dy, gamma, beta


#: the soft scores a VQA target holds: min(1, 0.3 * number of annotators who gave the answer)
SOFT_SCORES = (0.3, 0.6, 0.9, 1.0)


def bce_inputs(M, V, seed=0):
    """logits ~ 4 N(0, 1) with one +90 and two -90; targets: ~1 % of the entries carry a soft score, every second row also at
    its argmax (so the score is not trivially 0), the LAST row is all zero.  No row has a tied maximum (unique_argmax checks)."""
    g = torch.Generator().manual_seed(100003 * seed + 31 * M + V)
    logits = torch.randn((M, V), generator=g) * 4.0
    logits[0, 2 % V] = 90.0
    logits[min(1, M - 1), 3 % V] = -90.0
    logits[min(2, M - 1), 5 % V] = -90.0
    soft = torch.tensor(SOFT_SCORES)[torch.randint(0, len(SOFT_SCORES), (M, V), generator=g)]
    target = torch.where(torch.rand((M, V), generator=g) < 0.01, soft, torch.zeros(()))
    label = logits.argmax(1)
    for r in range(0, M, 2):
        target[r, label[r]] = SOFT_SCORES[r % len(SOFT_SCORES)]
        target[r, (3 * r + 1) % V] = 0.3
    target[M - 1] = 0.0
    return logits, target


def unique_argmax(logits):
    """every row's maximum is attained once"""
    m = logits.max(1, keepdim=True).values
    return bool(((logits == m).sum(1) == 1).all())


# ---- the head -------------------------------------------------------------------------------------------------------------------
HEAD_KEYS = ("logit_fc.0.weight", "logit_fc.0.bias", "logit_fc.2.weight", "logit_fc.2.bias", "logit_fc.3.weight", "logit_fc.3.bias")


def head_state(H, A, seed=0):
    """a state dict of BertVisualAnswerHead(hidden_size H, A answers) away from its initial values (fp32)"""
    g = torch.Generator().manual_seed(7919 * seed + H + A)
    return {
        "logit_fc.0.weight": torch.randn((2 * H, H), generator=g) * 0.05,
        "logit_fc.0.bias": torch.randn(2 * H, generator=g) * 0.1,
        "logit_fc.2.weight": 1.0 + 0.2 * torch.randn(2 * H, generator=g),
        "logit_fc.2.bias": torch.randn(2 * H, generator=g) * 0.1,
        "logit_fc.3.weight": torch.randn((A, 2 * H), generator=g) * 0.05,
        "logit_fc.3.bias": torch.randn(A, generator=g) * 0.1,
    }


def head_logits(sd, pooled):
    """BertVisualAnswerHead.forward on tensors of one dtype"""
    h = F.linear(pooled, sd["logit_fc.0.weight"], sd["logit_fc.0.bias"])
    h = bert_layer_norm(gelu(h), sd["logit_fc.2.weight"], sd["logit_fc.2.bias"])
    return F.linear(h, sd["logit_fc.3.weight"], sd["logit_fc.3.bias"])


def head_case(sd, pooled, dtype, target=None, labels=None):
    """the head with the VQA loss (target) or the pre-training QA loss (labels) in `dtype`:
    dict(logits, loss, score (target only), grads {key: gradient, "pooled": gradient})"""
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    x = pooled.detach().cpu().to(dtype).clone().requires_grad_(True)
    logits = head_logits(p, x)
    out = dict(logits=logits.detach())
    if target is not None:
        t = target.detach().cpu().to(dtype)
        loss = torch.nn.BCEWithLogitsLoss()(logits, t) * logits.size(1)
        _, label = logits.detach().max(1)
        out["score"] = t[torch.arange(logits.size(0)), label].mean()
    else:
        loss = torch.nn.CrossEntropyLoss(ignore_index=-1)(logits.view(-1, logits.size(-1)), labels.detach().cpu().view(-1))
    grads = torch.autograd.grad(loss, [p[k] for k in HEAD_KEYS] + [x])
    out["loss"] = loss.detach()
    out["grads"] = dict(zip(HEAD_KEYS + ("pooled",), grads))
    return out
