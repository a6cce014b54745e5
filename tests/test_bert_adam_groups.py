"""BertAdam with per-group hyper-parameters and every LR schedule evaluated on the device (vb_bert_adam_step_groups).

Arithmetic reference: oracle.visualbert_oracle.bert_adam_step, called once per group with that group's hyper-parameters
(names = the group's parameter names, schedule = a step -> multiplier callable).  Multiplier reference: the real reference's
own values in tests/golden/schedules.json (six classes, steps 0..43, t_total 40)."""
import copy
import ctypes
import io
import json
import os

import pytest
import torch

from oracle import visualbert_oracle as vo
from golden_util import GOLDEN_DIR, T_TOTAL, load_case, maxdiff
from test_model_parity import build_model, to_dev

gpu = pytest.mark.gpu

CHUNK = 16384
COLS = 11            # lr, b1, b2, eps, weight_decay, max_grad_norm, schedule code, warmup, t_total, cycles, host multiplier
VB_ERR_ARG = -1
# schedule codes of include/visualbert_hip.h
CODES = {"ConstantLR": 0, "WarmupLinearSchedule": 1, "WarmupConstantSchedule": 2, "WarmupCosineSchedule": 3,
         "WarmupCosineWithHardRestartsSchedule": 4, "WarmupCosineWithWarmupRestartsSchedule": 5}
HOST_CODE = 6


# ------------------------------------------------------------------------------------------------------------------------
# ABI level: a hand-made arena
# ------------------------------------------------------------------------------------------------------------------------
class Arena(object):
    """params / grads / moments / shadow of one flat layout + the two int64 tables of the optimizer entries."""

    def __init__(self, dev, sizes, offsets, flags, shadowed=()):
        self.dev, self.sizes, self.offsets = dev, list(sizes), list(offsets)
        total = max(o + n for o, n in zip(offsets, sizes))
        tens, chunks = [], []
        for i, (o, n) in enumerate(zip(offsets, sizes)):
            tens += [o, n, o if i in shadowed else -1, flags[i]]
            count = (n + CHUNK - 1) // CHUNK
            for s in range(0, n, CHUNK):
                chunks += [i, o + s, min(CHUNK, n - s), count]
        self.nt, self.nc = len(sizes), len(chunks) // 4
        self.tt = torch.tensor(tens, dtype=torch.int64).to(dev)
        self.ct = torch.tensor(chunks, dtype=torch.int64).to(dev)
        self.params = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grads = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.shadow = torch.zeros(total, dtype=torch.bfloat16, device=dev)
        self.norm2 = torch.zeros(self.nt + self.nc, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(self.nt, dtype=torch.int32, device=dev)

    def view(self, buf, i):
        return buf[self.offsets[i]:self.offsets[i] + self.sizes[i]]

    def snapshot(self):
        return [t.clone() for t in (self.params, self.m, self.v, self.shadow, self.steps)]

    def unchanged_since(self, snap):
        return all(torch.equal(a, b) for a, b in zip(snap, (self.params, self.m, self.v, self.shadow, self.steps)))

    def step_groups(self, table, n_groups, touched=None, validate=1, tt=None):
        from visualbert_amd import _lib
        rc = _lib.lib().vb_bert_adam_step_groups(
            _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m), _lib.ptr(self.v), _lib.ptr(self.shadow),
            _lib.ptr(self.ct), self.nc, _lib.ptr(self.tt if tt is None else tt), self.nt, _lib.ptr(touched),
            _lib.ptr(self.norm2), _lib.ptr(self.steps), _lib.ptr(table), n_groups, validate, _lib.stream_ptr())
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return rc

    def step_scalars(self, touched, lr, b1, b2, eps, wd, mgn, warmup, t_total, schedule):
        from visualbert_amd import _lib
        rc = _lib.lib().vb_bert_adam_step(
            _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m), _lib.ptr(self.v), _lib.ptr(self.shadow),
            _lib.ptr(self.ct), self.nc, _lib.ptr(self.tt), self.nt, _lib.ptr(touched), _lib.ptr(self.norm2),
            _lib.ptr(self.steps), lr, b1, b2, eps, wd, mgn, warmup, t_total, schedule, _lib.stream_ptr())
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return rc


def table_of(rows, dev):
    assert all(len(r) == COLS for r in rows)
    return torch.tensor([x for r in rows for x in r], dtype=torch.float64).to(dev)


def schedule_row(sch, lr=1.0, b1=0.0, b2=0.0, eps=0.0, wd=0.0, mgn=-1.0, code=None, mult=1.0):
    code = CODES[type(sch).__name__] if code is None else code
    return [lr, b1, b2, eps, wd, mgn, float(code), float(sch.warmup), float(sch.t_total),
            float(getattr(sch, "cycles", 0.0)), mult]


@gpu
def test_device_multipliers_match_the_reference_for_all_six_classes(dev):
    """p = 0, g = 1, lr = 1, b1 = b2 = 0, eps = 0, no decay, no clipping: -p after one launch is the kernel's fp32 multiplier.
    Bound 1.2e-7 = one fp32 ulp at 1.0: rounding a double in [0, 1] to fp32 costs at most 6e-8, the rest allows a last-bit
    difference of the device's double cos."""
    from visualbert_amd import optimization as opt
    fx = json.load(open(os.path.join(GOLDEN_DIR, "schedules.json")))
    assert len(fx["cases"]) == 6 and all(len(c["lr"]) == 44 for c in fx["cases"])
    rows, gid, start, want = [], [], [], []
    for gi, c in enumerate(fx["cases"]):
        sch = getattr(opt, c["schedule"])(t_total=fx["t_total"], **c["kwargs"])
        rows.append(schedule_row(sch))
        for s in range(44):
            gid.append(gi)
            start.append(s)
            want.append(c["lr"][s])
    # a seventh group: t_total = -1 gives exactly 1 whatever the class
    rows.append(schedule_row(opt.WarmupCosineSchedule(warmup=0.1, t_total=-1)))
    for s in (0, 7, 43):
        gid.append(6)
        start.append(s)
        want.append(1.0)
    n = len(gid)
    assert n == 264 + 3
    a = Arena(dev, [1] * n, list(range(n)), [1 | (g << 2) for g in gid])
    a.grads.fill_(1.0)
    a.steps.copy_(torch.tensor(start, dtype=torch.int32))
    assert a.step_groups(table_of(rows, dev), 7) == 0
    got = (-a.params).double().cpu()
    err = (got - torch.tensor(want, dtype=torch.float64)).abs()
    print("max |multiplier - golden| = %.3e" % float(err.max()))
    assert float(err.max()) <= 1.2e-7, (float(err.max()), int(err.argmax()))
    assert all(float(x) == 1.0 for x in got[264:])
    assert a.steps.cpu().tolist() == [s + 1 for s in start]


# the layout of the mixed-group tests: one chunk, a ragged last chunk (16389), an aligned multi-chunk tensor (32772 at a
# 16-byte-aligned offset), tensors at offsets 1 and 65813 (the scalar norm path), an 8 x 24 tensor with a bf16 shadow
SIZES = [1, 3, 64, 16384, 16389, 32772, 8 * 24, 5, 7]
OFFSETS = [0, 1, 4, 68, 16452, 32844, 65616, 65808, 65813]
SHADOWED = (6,)
FROZEN, UNTOUCHED = 7, 8            # flag bit 0 clear / touched = 0 with a zero gradient and a zero counter


def _mixed_groups():
    from visualbert_amd import optimization as opt
    return [dict(lr=1e-3, b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01, max_grad_norm=1.0,
                 schedule=opt.WarmupLinearSchedule(warmup=0.1, t_total=40)),
            dict(lr=2e-3, b1=0.8, b2=0.99, e=1e-8, weight_decay=0.05, max_grad_norm=-1.0,
                 schedule=opt.WarmupCosineSchedule(warmup=0.25, t_total=40, cycles=0.5)),
            dict(lr=5e-4, b1=0.85, b2=0.98, e=1e-5, weight_decay=0.0, max_grad_norm=0.05,
                 schedule=opt.WarmupLinearSchedule(warmup=0.25, t_total=20))]


MIXED_BOUND = 2 * 2.384e-7          # 2 x the measured maximum, see test_mixed_groups_match_the_oracle_per_group


def _rows(groups):
    return [schedule_row(g["schedule"], g["lr"], g["b1"], g["b2"], g["e"], g["weight_decay"], g["max_grad_norm"])
            for g in groups]


@gpu
def test_mixed_groups_match_the_oracle_per_group(dev):
    """three groups assigned round-robin (neighbouring tensors differ in group), differing in every column, three launches.
    Measured max |p - oracle| after the three launches: 2.384e-7 on the kernel-logic simulator (two fp32 ulps of a parameter
    near 1; the moments differ by 8.9e-8).  Asserted: 2 x that, below the 2e-6 of test_fp32_train_steps_match_reference_golden."""
    groups = _mixed_groups()
    n = len(SIZES)
    gid = [i % 3 for i in range(n)]
    flags = [(0 if i == FROZEN else 1) | (gid[i] << 2) for i in range(n)]
    a = Arena(dev, SIZES, OFFSETS, flags, SHADOWED)
    gen = torch.Generator().manual_seed(11)
    a.params.copy_(torch.rand(a.params.numel(), generator=gen) * 2 - 1)
    start = [0, 3, 6, 9, 12, 15, 18, 5, 0]
    a.steps.copy_(torch.tensor(start, dtype=torch.int32))
    a.view(a.m, FROZEN).copy_(torch.rand(SIZES[FROZEN], generator=gen))
    a.view(a.v, FROZEN).copy_(torch.rand(SIZES[FROZEN], generator=gen))
    names = ["t%d.weight" % i for i in range(n)]                   # no 'bias' / 'LayerNorm': the group's weight decay applies
    ref = {names[i]: a.view(a.params, i).cpu().clone() for i in range(n)}
    state = {names[i]: dict(step=start[i], next_m=torch.zeros(SIZES[i]), next_v=torch.zeros(SIZES[i])) for i in range(n)}
    frozen = [a.view(b, FROZEN).clone() for b in (a.params, a.m, a.v)]
    untouched = a.view(a.params, UNTOUCHED).clone()
    touched = torch.tensor([0.0 if i == UNTOUCHED else 1.0 for i in range(n)]).to(dev)
    table = table_of(_rows(groups), dev)
    live = [i for i in range(n) if i not in (FROZEN, UNTOUCHED)]
    for launch in range(3):
        g = torch.rand(a.grads.numel(), generator=gen) * 2 - 1
        a.grads.copy_(g)
        a.view(a.grads, UNTOUCHED).zero_()
        assert a.step_groups(table, 3, touched=touched, validate=1 if launch == 0 else 0) == 0
        grads = {names[i]: a.view(a.grads, i).cpu().clone() for i in live}
        for gi, gr in enumerate(groups):
            vo.bert_adam_step(ref, grads, state, gr["lr"], 0.0, -1, b1=gr["b1"], b2=gr["b2"], e=gr["e"],
                              weight_decay=gr["weight_decay"], max_grad_norm=gr["max_grad_norm"],
                              names=[names[i] for i in live if gid[i] == gi], schedule=gr["schedule"].get_lr)
    err = max(maxdiff(a.view(a.params, i).cpu(), ref[names[i]]) for i in live)
    merr = max(maxdiff(a.view(a.m, i).cpu(), state[names[i]]["next_m"]) for i in live)
    print("max |p - oracle| = %.3e   max |m - oracle| = %.3e" % (err, merr))
    assert err <= MIXED_BOUND, err
    assert MIXED_BOUND <= 2e-6
    o = OFFSETS[SHADOWED[0]]
    assert torch.equal(a.shadow[o:o + 192], a.params[o:o + 192].to(torch.bfloat16))
    assert a.steps.cpu().tolist() == [s + 3 for s in start[:7]] + [5, 0]
    for b, was in zip((a.params, a.m, a.v), frozen):                # flag bit 0 clear: bit-unchanged
        assert torch.equal(a.view(b, FROZEN), was)
    assert torch.equal(a.view(a.params, UNTOUCHED), untouched)       # never touched, zero gradient: no step, no weight decay
    assert float(a.view(a.m, UNTOUCHED).abs().max()) == 0.0


@gpu
def test_equal_rows_are_bit_identical_to_the_scalar_entry(dev):
    """a two-group table of equal rows against vb_bert_adam_step with the same scalars (warmup 0.25 and t_total 40 are exact
    in fp32, which is what the scalar entry carries them in)."""
    from visualbert_amd import optimization as opt
    n = len(SIZES)
    sch = opt.WarmupLinearSchedule(warmup=0.25, t_total=40)
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, mgn=1.0)
    row = schedule_row(sch, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["mgn"])
    gen = torch.Generator().manual_seed(5)
    p0 = torch.rand(OFFSETS[-1] + SIZES[-1], generator=gen) * 2 - 1
    gs = [torch.rand(p0.numel(), generator=gen) * 2 - 1 for _ in range(2)]
    touched = torch.ones(n).to(dev)
    results = []
    for grouped in (True, False):
        a = Arena(dev, SIZES, OFFSETS, [3 | ((i % 2) << 2 if grouped else 0) for i in range(n)], SHADOWED)
        a.params.copy_(p0)
        a.steps.copy_(torch.arange(n, dtype=torch.int32) * 5)
        for g in gs:
            a.grads.copy_(g)
            if grouped:
                assert a.step_groups(table_of([row, row], dev), 2, touched=touched) == 0
            else:
                assert a.step_scalars(touched, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["mgn"], 0.25, 40.0, 1) == 0
        results.append(a.snapshot())
    for x, y in zip(*results):
        assert torch.equal(x, y)
    assert results[0][4].cpu().tolist() == [5 * i + 2 for i in range(n)]


@gpu
def test_bad_tables_are_argument_errors_and_change_nothing(dev):
    n = len(SIZES)
    a = Arena(dev, SIZES, OFFSETS, [1 | ((i % 3) << 2) for i in range(n)], SHADOWED)
    gen = torch.Generator().manual_seed(3)
    a.params.copy_(torch.rand(a.params.numel(), generator=gen))
    a.grads.copy_(torch.rand(a.params.numel(), generator=gen))
    snap = a.snapshot()
    rows = _rows(_mixed_groups())
    good = table_of(rows, dev)
    assert a.step_groups(None, 3) == VB_ERR_ARG                                        # no table
    assert a.step_groups(good, 0) == VB_ERR_ARG                                        # no groups
    assert a.step_groups(good, 2) == VB_ERR_ARG                                        # tensors 2, 5, 8 name group 2
    bad = [list(r) for r in rows]
    bad[1][6] = 7.0
    assert a.step_groups(table_of(bad, dev), 3) == VB_ERR_ARG                          # unknown schedule code
    assert a.unchanged_since(snap)
    assert a.step_groups(good, 3) == 0 and not a.unchanged_since(snap)


# ------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------
NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight"]


def _four_group_specs(model):
    """encoder decay / no-decay and head decay / no-decay, as the issue lists them.  Names are the oracle's (model.bert's)."""
    from visualbert_amd import optimization as opt
    named = [(n, p) for n, p in model.bert.named_parameters() if "pooler" not in n]
    enc = dict(lr=1e-3, b1=0.9, b2=0.999, e=1e-6, max_grad_norm=1.0)
    head = dict(lr=5e-3, b1=0.8, b2=0.999, e=1e-6, max_grad_norm=0.5)
    specs = []
    for is_head, hp, wd in ((False, enc, 0.01), (True, head, 0.05)):
        for nodecay in (False, True):
            names = [n for n, _ in named if (not n.startswith("bert.")) == is_head and
                     any(nd in n for nd in NO_DECAY) == nodecay]
            sch = opt.WarmupCosineSchedule(warmup=0.1, t_total=T_TOTAL) if is_head else opt.WarmupLinearSchedule(0.1, T_TOTAL)
            specs.append(dict(hp, names=names, weight_decay=0.0 if nodecay else wd, schedule=sch))
    assert all(s["names"] for s in specs)
    return specs


def _optimizer_groups(model, specs):
    named = dict(model.bert.named_parameters())
    return [dict({k: v for k, v in s.items() if k != "names"}, params=[named[n] for n in s["names"]]) for s in specs]


def _oracle_step(ref_sd, state, cfg, head, batch, specs):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in ref_sd.items()}
    ro = vo.objective_forward(leaves, cfg, head, mode="fp32", **batch)
    ro["loss"].backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    with torch.no_grad():
        for s in specs:
            vo.bert_adam_step(ref_sd, grads, state, s["lr"], 0.0, -1, b1=s["b1"], b2=s["b2"], e=s["e"],
                              weight_decay=s["weight_decay"], max_grad_norm=s["max_grad_norm"], names=s["names"],
                              schedule=s["schedule"].get_lr)
    return float(ro["loss"].detach())


def _model_step(model, optim, b):
    optim.zero_grad()
    out = model(**b)
    out["loss"].backward()
    optim.step()
    return float(out["loss"].detach())


def _assert_weights(model, ref_sd, bound=5e-6):
    for n, p in model.bert.named_parameters():
        assert maxdiff(p.detach().cpu(), ref_sd[n]) < bound, n


@gpu
def test_four_groups_follow_the_oracle(dev):
    """the bounds of test_bert_adam_host_evaluated_schedules, which this mirrors: loss within 1e-4, weights within 5e-6"""
    from visualbert_amd import optimization as opt
    cfg, head, sd, batch, g = load_case("micro_nlvr")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    specs = _four_group_specs(model)
    optim = opt.BertAdam(_optimizer_groups(model, specs), lr=1e-3)
    ref_sd, state, b = copy.deepcopy(sd), {}, to_dev(batch, dev)
    for step in range(4):
        loss = _model_step(model, optim, b)
        assert abs(loss - _oracle_step(ref_sd, state, cfg, head, batch, specs)) < 1e-4, step
    _assert_weights(model, ref_sd)
    st = optim.state_dict()["state"]
    order = [n for s in specs for n in s["names"]]
    assert [st[k]["step"] for k in range(len(order))] == [state[n]["step"] if n in state else 0 for n in order]
    assert st[0]["step"] == 4 and min(s["step"] for s in st.values()) == 4
    want = []
    member = {id(p): gr for gr in optim.param_groups for p in gr["params"]}
    for p in model.bert.arena.params:
        if id(p) in member:
            want.append(member[id(p)]["lr"] * member[id(p)]["schedule"].get_lr(4))
    assert optim.get_lr() == want and len(set(want)) == 2
    _model_step(model, optim, b)
    assert optim.table_uploads == 1                     # five steps of an unchanged configuration: one upload


@gpu
def test_changing_a_group_between_steps_takes_effect_at_the_next_step(dev):
    from visualbert_amd import optimization as opt
    cfg, head, sd, batch, g = load_case("micro_nlvr")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    specs = _four_group_specs(model)
    optim = opt.BertAdam(_optimizer_groups(model, specs), lr=1e-3)
    ref_sd, state, b = copy.deepcopy(sd), {}, to_dev(batch, dev)
    for step in range(4):
        if step == 2:
            optim.param_groups[0]["lr"] *= 0.5
            optim.param_groups[2]["max_grad_norm"] = 0.01
            specs[0]["lr"] *= 0.5
            specs[2]["max_grad_norm"] = 0.01
        loss = _model_step(model, optim, b)
        assert abs(loss - _oracle_step(ref_sd, state, cfg, head, batch, specs)) < 1e-4, step
    _assert_weights(model, ref_sd)
    assert optim.table_uploads == 2
    # the same steps WITHOUT the change end somewhere else: the change is what the comparison above saw
    specs2 = _four_group_specs(model)
    ref2, state2 = copy.deepcopy(sd), {}
    for step in range(4):
        _oracle_step(ref2, state2, cfg, head, batch, specs2)
    assert max(maxdiff(ref2[n], ref_sd[n]) for n in specs[0]["names"]) > 1e-4


@gpu
def test_checkpoint_round_trip_per_group(dev):
    """two groups with their own cosine schedules, tensors at different step counts: save, load into a fresh model and a
    freshly (and differently) configured optimizer, one more step on both -- within 1e-7, as
    test_checkpoint_round_trip_resumes_identically asks."""
    from visualbert_amd import optimization as opt
    cfg, head, sd, batch, g = load_case("micro_pretraining")
    text_only = {k: v for k, v in batch.items() if not k.startswith("image_")}

    def make(weights, configured):
        model = build_model(cfg, head, weights, dev, dropout=0.0)
        model.train()
        named = [(n, p) for n, p in model.bert.named_parameters() if "pooler" not in n]
        dec = [p for n, p in named if not any(nd in n for nd in NO_DECAY)]
        nod = [p for n, p in named if any(nd in n for nd in NO_DECAY)]
        if not configured:
            return model, opt.BertAdam([{"params": dec}, {"params": nod}], lr=1.0, warmup=0.5, t_total=7)
        groups = [dict(params=dec, lr=1e-3, weight_decay=0.01,
                       schedule=opt.WarmupCosineWithWarmupRestartsSchedule(warmup=0.05, t_total=T_TOTAL, cycles=4.)),
                  dict(params=nod, lr=2e-3, weight_decay=0.0, b1=0.8, max_grad_norm=0.5,
                       schedule=opt.WarmupCosineSchedule(warmup=0.1, t_total=T_TOTAL))]
        return model, opt.BertAdam(groups, lr=1e-3)

    model, optim = make(sd, True)
    assert optim.param_groups[0]["schedule"].warmup == 0.2
    _model_step(model, optim, to_dev(text_only, dev))       # the visual tables take no step here ...
    _model_step(model, optim, to_dev(batch, dev))           # ... and their first one here
    saved = optim.state_dict()
    assert sorted(set(s["step"] for s in saved["state"].values())) == [1, 2]
    buf = io.BytesIO()
    torch.save({"optimizer": saved, "model": {k: v.cpu() for k, v in model.bert.state_dict().items()}}, buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    model2, optim2 = make({k: v for k, v in ck["model"].items() if k in sd}, False)
    optim2.load_state_dict(ck["optimizer"])
    for ga, gb in zip(optim.param_groups, optim2.param_groups):
        assert type(ga["schedule"]) is type(gb["schedule"])
        for k in ("warmup", "t_total", "cycles"):
            assert getattr(ga["schedule"], k) == getattr(gb["schedule"], k), k
        for k in ("lr", "b1", "b2", "e", "weight_decay", "max_grad_norm"):
            assert ga[k] == gb[k], k
    assert optim2.param_groups[0]["schedule"].warmup == 0.2 and optim2.param_groups[0]["schedule"].cycles == 4.
    again = optim2.state_dict()
    assert [s["step"] for s in again["state"].values()] == [s["step"] for s in saved["state"].values()]
    b = to_dev(batch, dev)
    la, lb = _model_step(model, optim, b), _model_step(model2, optim2, b)
    assert abs(la - lb) < 1e-6
    for (n, p), (_, q) in zip(model.bert.named_parameters(), model2.bert.named_parameters()):
        assert maxdiff(p.detach().cpu(), q.detach().cpu()) < 1e-7, n
    assert optim.get_lr() == optim2.get_lr()


@gpu
def test_user_schedule_beside_a_device_schedule(dev):
    """a user subclass of _LRSchedule has no device formula: its group's multiplier comes from the host each step"""
    from visualbert_amd import optimization as opt

    class Hyperbolic(opt._LRSchedule):
        def get_lr_(self, progress):
            return 1. / (1. + 10. * progress)

    cfg, head, sd, batch, g = load_case("micro_nlvr")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    named = [(n, p) for n, p in model.bert.named_parameters() if "pooler" not in n]
    hp = dict(b1=0.9, b2=0.999, e=1e-6, max_grad_norm=1.0)
    specs = [dict(hp, lr=1e-3, weight_decay=0.01, schedule=opt.WarmupLinearSchedule(0.1, T_TOTAL),
                  names=[n for n, _ in named if not any(nd in n for nd in NO_DECAY)]),
             dict(hp, lr=2e-3, weight_decay=0.0, schedule=Hyperbolic(warmup=0.0, t_total=10),
                  names=[n for n, _ in named if any(nd in n for nd in NO_DECAY)])]
    optim = opt.BertAdam(_optimizer_groups(model, specs), lr=1e-3)
    ref_sd, state, b = copy.deepcopy(sd), {}, to_dev(batch, dev)
    for step in range(2):
        loss = _model_step(model, optim, b)
        assert abs(loss - _oracle_step(ref_sd, state, cfg, head, batch, specs)) < 1e-4, step
    _assert_weights(model, ref_sd)
    assert optim.table_uploads == 2                       # the host multiplier moved between the two steps
    assert set(optim.get_lr()) == {1e-3 * specs[0]["schedule"].get_lr(2), 2e-3 * (1. / (1. + 10. * (2. / 10)))}


@gpu
def test_group_added_after_a_step_keeps_the_earlier_state(dev):
    from visualbert_amd import optimization as opt
    cfg, head, sd, batch, g = load_case("micro_nlvr")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    specs = _four_group_specs(model)
    groups = _optimizer_groups(model, specs)
    optim = opt.BertAdam(groups[:2], lr=1e-3)              # the encoder only
    b = to_dev(batch, dev)
    _model_step(model, optim, b)
    before = optim.state_dict()["state"]
    n_before = len(before)
    head_before = {n: p.detach().clone() for n, p in model.bert.named_parameters() if n in specs[2]["names"]}
    optim.add_param_group(groups[2])
    after = optim.state_dict()["state"]
    assert len(after) == n_before + len(specs[2]["names"])
    assert before[0]["step"] == 1
    for k in range(n_before):
        assert after[k]["step"] == before[k]["step"]
        assert torch.equal(after[k]["next_m"], before[k]["next_m"]) and torch.equal(after[k]["next_v"], before[k]["next_v"])
    assert float(max(s["next_v"].abs().max() for s in before.values())) > 0
    assert all(after[k]["step"] == 0 and float(after[k]["next_m"].abs().max()) == 0 for k in range(n_before, len(after)))
    for n, p in model.bert.named_parameters():              # not optimised so far
        if n in head_before:
            assert torch.equal(p.detach(), head_before[n])
    _model_step(model, optim, b)
    steps = [s["step"] for s in optim.state_dict()["state"].values()]
    assert steps[:n_before] == [before[k]["step"] + 1 for k in range(n_before)]
    assert steps[n_before:] == [1] * len(specs[2]["names"])
    # (the new group's first step is step 0 of its warm-up: multiplier 0, so its weights stand still; its moments do not)
    late = list(optim.state_dict()["state"].values())[n_before:]
    assert all(float(s["next_v"].abs().max()) > 0 for s in late)


# ------------------------------------------------------------------------------------------------------------------------
# the group helper
# ------------------------------------------------------------------------------------------------------------------------
def _three_layer_names():
    from visualbert_amd.modeling import BertConfig, TrainVisualBERTObjective
    cfg = vo.OracleConfig(**vo.CONFIGS["micro"])
    bc = BertConfig(cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=3,
                    num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size)
    m = TrainVisualBERTObjective(bc, "nlvr", visual_embedding_dim=cfg.visual_embedding_dim)
    return [n for n, _ in m.named_parameters()]


def test_layerwise_groups_on_real_parameter_names():
    from visualbert_amd.optimization import layerwise_groups
    names = _three_layer_names()
    assert any("pooler" in n for n in names) and any(n.startswith("bert.encoder.layer.2.") for n in names)
    pairs = [(n, torch.zeros(1)) for n in names]
    name_of = {id(t): n for n, t in pairs}
    lr, decay, head_lr = 1e-3, 0.9, 4e-3
    groups = layerwise_groups(pairs, lr, layer_decay=decay, head_lr=head_lr, weight_decay=0.01)
    seen = [name_of[id(t)] for g in groups for t in g["params"]]
    assert sorted(seen) == sorted(n for n in names if "pooler" not in n)             # every name exactly once
    ref_decay, ref_nodecay = vo.optimizer_groups(names)
    for g in groups:
        for t in g["params"]:
            n = name_of[id(t)]
            if n.startswith("bert.embeddings."):
                want = lr * decay ** 3
            elif n.startswith("bert.encoder.layer."):
                want = lr * decay ** (3 - 1 - int(n.split(".")[3]))
            else:
                want = head_lr
            assert g["lr"] == want, n
            assert g["weight_decay"] == (0.01 if n in ref_decay else 0.0), n
            assert (n in ref_decay) != (n in ref_nodecay)
    assert len(set(g["lr"] for g in groups)) == 5                                   # embeddings, three layers, the heads
    # no decay, no head lr: today's two groups, in today's order
    plain = layerwise_groups(pairs, lr)
    merged = {}
    for g in plain:
        merged.setdefault((g["lr"], g["weight_decay"]), []).extend(name_of[id(t)] for t in g["params"])
    assert merged == {(lr, 0.01): ref_decay, (lr, 0.0): ref_nodecay}


def _wrapper(dev, **extra):
    from visualbert_amd.model import ModelWrapper, AttrDict
    cfg, head, sd, batch, g = load_case("micro_nlvr")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    args = AttrDict(train_batch_size=1, learning_rate=1e-3, warmup_proportion=0.1, num_train_epochs=1,
                    gradient_accumulation_steps=1, **extra)
    return ModelWrapper(args, T_TOTAL, model=model), model, (cfg, head, sd, batch)


@gpu
def test_wrapper_without_the_new_keys_builds_the_two_groups(dev):
    mw, model, _ = _wrapper(dev)
    named = [(n, p) for n, p in model.named_parameters() if "pooler" not in n]
    groups = mw.optimizer.param_groups
    assert len(groups) == 2
    assert [id(p) for p in groups[0]["params"]] == [id(p) for n, p in named if not any(nd in n for nd in NO_DECAY)]
    assert [id(p) for p in groups[1]["params"]] == [id(p) for n, p in named if any(nd in n for nd in NO_DECAY)]
    assert (groups[0]["weight_decay"], groups[1]["weight_decay"]) == (0.01, 0.0)
    assert groups[0]["lr"] == groups[1]["lr"] == 1e-3
    # this set-up is one the scalar entry expresses: no group table is made for it, until a group is given its own value
    b = to_dev(load_case("micro_nlvr")[3], dev)
    mw.step(b)
    assert mw.optimizer.table_uploads == 0
    groups[1]["lr"] = 2e-3
    mw.step(b)
    assert mw.optimizer.table_uploads == 1
    assert sorted(set(mw.optimizer.get_lr())) == sorted(g["lr"] * g["schedule"].get_lr(2) for g in groups)


@gpu
def test_wrapper_with_layerwise_decay_follows_the_oracle(dev):
    mw, model, (cfg, head, sd, batch) = _wrapper(dev, layerwise_lr_decay=0.9)
    name_of = {id(p): n for n, p in model.bert.named_parameters()}
    specs = []
    for g in mw.optimizer.param_groups:
        specs.append(dict(names=[name_of[id(p)] for p in g["params"]], lr=g["lr"], b1=g["b1"], b2=g["b2"], e=g["e"],
                          weight_decay=g["weight_decay"], max_grad_norm=g["max_grad_norm"], schedule=g["schedule"]))
    L = cfg.num_hidden_layers
    assert sorted(set(s["lr"] for s in specs)) == sorted(set(1e-3 * 0.9 ** k for k in range(L + 1)))
    ref_sd, state, b = copy.deepcopy(sd), {}, to_dev(batch, dev)
    for step in range(2):
        out = mw.step(b)
        assert abs(float(out["loss"].detach()) - _oracle_step(ref_sd, state, cfg, head, batch, specs)) < 1e-4, step
    _assert_weights(model, ref_sd)
