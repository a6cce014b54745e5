#!/usr/bin/env python
"""vb_lamb_step_groups next to vb_bert_adam_step_groups on the BERT-base parameter arena (111.5 M optimised parameters, the two
groups ModelWrapper builds), on the GPU box.  Both entries run on the same arena, tables and gradients, from the same process
image: each leg is a child process of its own under its own time limit (a leg that fails ends the run), the legs alternate
(adam, lamb, adam, lamb, ...) and every leg times `--iters` steps between two device events after `--warmup` steps.
The expectation is derived from bytes, as optim.hip counts them (per optimised parameter: BertAdam 28 B + 2 B per shadowed
element, LAMB 40 B + 2 B, minus 4 B where the trust ratio is 1 by rule; the gradient-norm pass adds 4 B to either):
    LAMB time <= (LAMB bytes / BertAdam bytes) x BertAdam time x 1.15
usage: python tools/lamb_bench.py [--rounds 3] [--iters 50] [--warmup 10] [--leg-timeout 180] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(kind, iters, warmup):
    import torch
    from visualbert_amd import _lib
    from visualbert_amd.modeling import BertConfig
    from visualbert_amd.model import VisualBERTFixedImageEmbedding
    from visualbert_amd import optimization as opt
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = VisualBERTFixedImageEmbedding(config=BertConfig(30522), training_head_type="pretraining",
                                          visual_embedding_dim=2048, compute_dtype=torch.bfloat16).to(dev)
    named = [(n, p) for n, p in model.named_parameters() if "pooler" not in n]
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    groups = [{"params": [p for n, p in named if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
              {"params": [p for n, p in named if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]
    cls = opt.Lamb if kind == "lamb" else opt.BertAdam
    optim = cls(groups, lr=1e-4, warmup=0.1, t_total=100000)
    f = optim.fused()
    a = f["arena"]
    a.grad.normal_(0.0, 1e-3)
    touched = torch.ones(f["nt"], device=dev)
    table = torch.tensor(optim._group_rows(f), dtype=torch.float64).to(dev)
    L = _lib.lib()
    fn = L.vb_lamb_step_groups if kind == "lamb" else L.vb_bert_adam_step_groups
    args = (_lib.ptr(a.data), _lib.ptr(a.grad), _lib.ptr(f["m"]), _lib.ptr(f["v"]), _lib.ptr(a.shadow), _lib.ptr(f["ct"]),
            f["nc"], _lib.ptr(f["tt"]), f["nt"], _lib.ptr(touched), _lib.ptr(f["norm2"]), _lib.ptr(f["steps"]),
            _lib.ptr(table), len(groups))
    _lib.check(fn(*args, 1, _lib.stream_ptr()), kind)                    # the tables are checked once
    for _ in range(warmup):
        _lib.check(fn(*args, 0, _lib.stream_ptr()), kind)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(*args, 0, _lib.stream_ptr())
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    # bytes per step from the tables
    n_opt = sum(p.numel() for g in groups for p in g["params"])
    n_shadow = sum(p.numel() for g in groups for p in g["params"] if p.dim() == 2)
    n_plain = sum(p.numel() for p in groups[1]["params"])              # LAMB: ratio 1 by rule, pass 2 does not read p
    update = 28 * n_opt + 2 * n_shadow if kind != "lamb" else 40 * n_opt + 2 * n_shadow - 4 * n_plain
    finite = bool(torch.isfinite(a.data).all())
    print(json.dumps(dict(leg=kind, us=us, n_opt=n_opt, n_chunks=f["nc"], n_tensors=f["nt"], update_bytes=update,
                          norm_bytes=4 * n_opt, steps=int(f["steps"].max()), finite=finite)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["adam", "lamb"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--leg-timeout", type=float, default=180.0)
    ap.add_argument("--out")
    o = ap.parse_args()
    if o.leg:
        return leg(o.leg, o.iters, o.warmup)
    runs = {"adam": [], "lamb": []}
    for _ in range(o.rounds):
        for kind in ("adam", "lamb"):
            # a fresh child per leg, never a retry: a leg that fails, faults or runs out of time ends the whole run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--iters", str(o.iters),
                                "--warmup", str(o.warmup)], stdout=subprocess.PIPE, timeout=o.leg_timeout)
            if r.returncode != 0:
                sys.exit("lamb_bench: leg %s ended with status %d" % (kind, r.returncode))
            rec = json.loads(r.stdout.decode().strip().splitlines()[-1])
            assert rec["finite"] and rec["steps"] == 1 + o.warmup + o.iters, rec
            runs[kind].append(rec)
            print("# %s %.1f us" % (kind, rec["us"]), file=sys.stderr)
    med = {k: sorted(x["us"] for x in v)[len(v) // 2] for k, v in runs.items()}
    ad, la = runs["adam"][0], runs["lamb"][0]
    ratio_update = la["update_bytes"] / ad["update_bytes"]
    ratio_total = (la["update_bytes"] + la["norm_bytes"]) / (ad["update_bytes"] + ad["norm_bytes"])
    out = dict(n_opt=ad["n_opt"], n_chunks=ad["n_chunks"], n_tensors=ad["n_tensors"], iters=o.iters, warmup=o.warmup,
               adam_us=[x["us"] for x in runs["adam"]], lamb_us=[x["us"] for x in runs["lamb"]],
               adam_us_median=med["adam"], lamb_us_median=med["lamb"],
               adam_bytes_per_param=ad["update_bytes"] / ad["n_opt"], lamb_bytes_per_param=la["update_bytes"] / la["n_opt"],
               norm_bytes_per_param=4.0, byte_ratio_update_passes=ratio_update, byte_ratio_with_norm_pass=ratio_total,
               measured_ratio=med["lamb"] / med["adam"],
               target_us_update_passes=ratio_update * med["adam"] * 1.15, target_us_with_norm_pass=ratio_total * med["adam"] * 1.15,
               adam_tb_per_s=(ad["update_bytes"] + ad["norm_bytes"]) / med["adam"] / 1e6,
               lamb_tb_per_s=(la["update_bytes"] + la["norm_bytes"]) / med["lamb"] / 1e6)
    out["meets_target"] = med["lamb"] <= out["target_us_update_passes"]
    out["meets_target_with_norm_pass"] = med["lamb"] <= out["target_us_with_norm_pass"]
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
