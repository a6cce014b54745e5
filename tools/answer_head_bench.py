#!/usr/bin/env python
"""Answer head (lxrt.BertVisualAnswerHead + the VQA loss) forward + backward against the same head written in plain PyTorch eager on
the same device: pooled batch 1024, H = 768, 3129 answers, bf16.  Writes both times to profiles/answer_head_bench.json:
python tools/answer_head_bench.py [--batch 1024] [--out profiles/answer_head_bench.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from torch import nn
from visualbert_amd import lxrt
from visualbert_amd.modeling import BertConfig

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--hidden", type=int, default=768)
ap.add_argument("--answers", type=int, default=3129)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "answer_head_bench.json"))
args = ap.parse_args()
B, H, V = args.batch, args.hidden, args.answers
dev = torch.device("cuda", 0)
dt = torch.bfloat16
g = torch.Generator().manual_seed(0)
pooled = torch.tanh(torch.randn(B, H, generator=g)).to(dt).to(dev)
target = torch.where(torch.rand(B, V, generator=g) < 0.01, torch.full((), 0.6), torch.zeros(())).to(dev)

head = lxrt.BertVisualAnswerHead(BertConfig(96, hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64,
                                            intermediate_size=4 * H), V)
head.apply(lxrt.lxrt_init_weights)
head = head.to(dev)
eager = nn.Sequential(nn.Linear(H, 2 * H), nn.GELU(), nn.LayerNorm(2 * H, eps=1e-12), nn.Linear(2 * H, V)).to(dev)
with torch.no_grad():
    for i in (0, 2, 3):
        eager[i].weight.copy_(head.logit_fc[i].weight)
        eager[i].bias.copy_(head.logit_fc[i].bias)
eager = eager.to(dt)
bce = nn.BCEWithLogitsLoss()


def step_hip():
    x = pooled.detach().requires_grad_(True)
    _, loss, _ = head(x, target=target)
    loss.backward()
    return loss


def step_eager():
    x = pooled.detach().requires_grad_(True)
    logit = eager(x).float()
    loss = bce(logit, target) * logit.size(1)
    loss.backward()
    return loss


def timed(fn, params):
    for _ in range(5):
        fn()
    for p in params:
        p.grad = None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3


l_hip, l_eager = float(step_hip().detach()), float(step_eager().detach())
t_hip = timed(step_hip, list(head.parameters()))
t_eager = timed(step_eager, list(eager.parameters()))
res = dict(batch=B, hidden=H, answers=V, dtype="bf16", iters=args.iters, device=torch.cuda.get_device_name(0),
           hip_fwd_bwd_us=t_hip, eager_fwd_bwd_us=t_eager, loss_hip=l_hip, loss_eager=l_eager)
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
