#!/usr/bin/env python
"""Masked-region objective kernel (vb_visual_loss_fwd_bwd) on the GPU box at M = 1024 x 36 regions and the real widths
(1600 | 400 | 2048, pitch 4096), bf16 and fp32, HIP events -- beside the same formula as PyTorch eager on the same card, forward +
backward.  Bytes moved = what the kernel touches: the vectors of the segments whose weight is not zero, the fp32 target of the rows
whose feature mask is 1, the whole gradient matrix; as a fraction of the 6.3 TB/s a streaming kernel achieves on MI355X.
usage: python tools/visual_loss_bench.py [output file]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from visualbert_amd import _lib

dev = torch.device("cuda", 0)
L = _lib.lib()
M, NO, NA, NF, LD = 1024 * 36, 1600, 400, 2048, 4096
W = 1 / 0.15
ACHIEVABLE = 6.3e12
g = torch.Generator().manual_seed(0)


def labels(n):
    lab = torch.randint(0, n, (M,), generator=g, dtype=torch.int64)
    lab[torch.rand(M, generator=g) < 0.2] = -1
    return lab


def conf():
    c = torch.rand(M, generator=g)
    c[torch.rand(M, generator=g) < 0.3] = 0.0
    return c


ol, oc, al, ac = labels(NO), conf(), labels(NA), conf()
fm = (torch.rand(M, generator=g) < 0.15).float()
on_o, on_a, on_f = (ol >= 0) & (oc != 0), (al >= 0) & (ac != 0), fm != 0
ol, oc, al, ac, fm = [t.to(dev) for t in (ol, oc, al, ac, fm)]
target = torch.randn((M, NF), device=dev)
ws = torch.empty(L.vb_visual_loss_ws_floats(M), device=dev)
losses = torch.empty(4, device=dev)


def bench(fn, iters=200):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def eager(scores):
    x = scores.detach().requires_grad_(True)
    xf = x.float()
    lo = (F.cross_entropy(xf[:, :NO], ol, ignore_index=-1, reduction="none") * oc).mean() * W
    la = (F.cross_entropy(xf[:, NO:NO + NA], al, ignore_index=-1, reduction="none") * ac).mean() * W
    lf = (F.smooth_l1_loss(xf[:, NO + NA:NO + NA + NF], target, reduction="none").mean(1) * fm).mean() * W
    (lo + la + lf).backward()
    return x.grad


lines = ["M = %d rows, widths %d | %d | %d, pitch %d; rows counted: obj %.0f %%, attr %.0f %%, feat %.0f %%, none %.0f %%"
         % (M, NO, NA, NF, LD, 100 * float(on_o.float().mean()), 100 * float(on_a.float().mean()), 100 * float(on_f.float().mean()),
            100 * float((~(on_o | on_a | on_f)).float().mean()))]
for dt in (torch.bfloat16, torch.float32):
    es = 2 if dt == torch.bfloat16 else 4
    scores = (torch.randn((M, LD), device=dev) * 3.0).to(dt)
    dscores = torch.empty_like(scores)
    call = lambda: L.vb_visual_loss_fwd_bwd(_lib.dtype_code(dt), _lib.ptr(scores), LD, NO, NA, NF, _lib.ptr(ol), _lib.ptr(oc), _lib.ptr(al),
                                            _lib.ptr(ac), _lib.ptr(target), NF, _lib.ptr(fm), W, W, W, _lib.ptr(ws), _lib.ptr(losses),
                                            _lib.ptr(dscores), LD, M, _lib.stream_ptr())
    assert call() == 0
    t_k = bench(call)
    t_e = bench(lambda: eager(scores), iters=20)
    read = (int(on_o.sum()) * NO + int(on_a.sum()) * NA + int(on_f.sum()) * NF) * es + int(on_f.sum()) * NF * 4 + M * 36
    write = M * LD * es + 3 * M * 4
    bw = (read + write) / (t_k * 1e-6)
    lines.append("%s: kernel %.1f us (reads %.0f MB, writes %.0f MB -> %.2f TB/s = %.0f %% of 6.3 TB/s) | PyTorch eager forward + backward "
                 "%.1f us | eager / kernel %.1fx" % ("bf16" if es == 2 else "fp32", t_k, read / 1e6, write / 1e6, bw / 1e12,
                                                     100 * bw / ACHIEVABLE, t_e, t_e / t_k))
    del scores, dscores
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
