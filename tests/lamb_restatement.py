"""LAMB as include/visualbert_hip.h states it for vb_lamb_step_groups, in plain PyTorch -- the yardstick of tests/test_lamb.py.
No LAMB exists in the reference tree, so the definition is restated here and run twice: in fp64 (the reference) and in fp32 (its
distance from the fp64 run sizes the tolerance: what fp32 arithmetic costs on these very numbers, whatever the order of the sums)."""
import math

import torch


def lamb_step(P, M, V, S, G, live, gid, groups, dtype):
    """one step, in place on the lists P, M, V (tensors of `dtype`) and S (step counters, ints), for the tensors `live` (the
    optimised, non-skipped ones, in table order).  G: the gradients; gid: group index per tensor; groups: dicts with lr, b1, b2,
    e, weight_decay, max_grad_norm, schedule (an object with get_lr(step)), bias_correction, always_adapt."""
    def c(x):
        return torch.tensor(float(x), dtype=dtype)

    g = {i: G[i].detach().cpu().to(dtype) for i in live}
    gnorm2 = c(0.0)
    for i in live:
        gnorm2 = gnorm2 + (g[i] * g[i]).sum()
    gnorm = torch.sqrt(gnorm2)
    for i in live:
        h = groups[gid[i]]
        b1, b2, eps, wd = c(h["b1"]), c(h["b2"]), c(h["e"]), c(h["weight_decay"])
        clip = c(1.0)
        if h["max_grad_norm"] > 0:
            clip = torch.clamp(c(h["max_grad_norm"]) / (gnorm + c(1e-6)), max=1.0)
        gi = g[i] * clip
        M[i] = M[i] * b1 + (1 - b1) * gi
        V[i] = V[i] * b2 + (1 - b2) * gi * gi
        mh, vh = M[i], V[i]
        if h["bias_correction"]:
            t = S[i] + 1
            mh = mh / c(1.0 - float(b1) ** t)
            vh = vh / c(1.0 - float(b2) ** t)
        u = mh / (torch.sqrt(vh) + eps)
        if h["weight_decay"] > 0:
            u = u + wd * P[i]
        r = c(1.0)
        if h["weight_decay"] > 0 or h["always_adapt"]:
            pn, un = torch.sqrt((P[i] * P[i]).sum()), torch.sqrt((u * u).sum())
            if float(pn) > 0 and float(un) > 0:
                r = pn / un
        P[i] = P[i] - c(h["lr"]) * c(h["schedule"].get_lr(S[i])) * r * u
        S[i] += 1


def ulp32(x):
    """the spacing of fp32 numbers at |x|"""
    x = abs(float(x))
    if x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def excess(got, r32, r64):
    """max |got - fp64| over its bound 4 x max |fp32 restatement - fp64| + 2 ulp(max |x|); a value <= 1 is within the bound"""
    got, r32 = got.detach().cpu().double().reshape(-1), r32.double().reshape(-1)
    r64 = r64.reshape(-1)
    bound = 4.0 * float((r32 - r64).abs().max()) + 2.0 * ulp32(float(r64.abs().max()))
    return float((got - r64).abs().max()) / bound
