"""The fused multi-tensor LAMB (vb_lamb_step_groups, visualbert_amd.optimization.Lamb, ModelWrapper's `optimizer: "lamb"`).

Yardstick: tests/lamb_restatement.py, the algorithm of include/visualbert_hip.h in plain PyTorch, run in fp64 and a second time in
fp32.  Per tensor and buffer (params, exp_avg, exp_avg_sq) the bound is
    max |kernel - fp64| <= 4 x max |fp32 restatement - fp64| + 2 ulp(max |x|)
(the factor 4 covers the different summation order of the norms); `excess` is the left side over the right side."""
import copy
import io

import pytest
import torch

from golden_util import T_TOTAL, load_case
from lamb_restatement import excess, lamb_step
from test_bert_adam_groups import Arena, CODES, VB_ERR_ARG
from test_bert_adam_groups import table_of as adam_table_of
from test_model_parity import build_model, to_dev

gpu = pytest.mark.gpu

COLS = 13            # the 11 columns of BertAdam's table, then bias_correction and always_adapt


class LambArena(Arena):
    def __init__(self, dev, sizes, offsets, flags, shadowed=()):
        from visualbert_amd import _lib
        super(LambArena, self).__init__(dev, sizes, offsets, flags, shadowed)
        n = _lib.lib().vb_lamb_ws_floats(self.nt, self.nc)
        assert 0 < n <= 8 * (self.nt + self.nc) + 64          # per-chunk and per-tensor scalars only
        self.ws = torch.zeros(n, dtype=torch.float32, device=dev)

    def step_lamb(self, table, n_groups, touched=None, validate=1, tt=None):
        from visualbert_amd import _lib
        rc = _lib.lib().vb_lamb_step_groups(
            _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m), _lib.ptr(self.v), _lib.ptr(self.shadow),
            _lib.ptr(self.ct), self.nc, _lib.ptr(self.tt if tt is None else tt), self.nt, _lib.ptr(touched),
            _lib.ptr(self.ws), _lib.ptr(self.steps), _lib.ptr(table), n_groups, validate, _lib.stream_ptr())
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        return rc

    def restore(self, snap):
        for t, s in zip((self.params, self.m, self.v, self.shadow, self.steps), snap):
            t.copy_(s)


def row_of(g):
    sch = g["schedule"]
    return [g["lr"], g["b1"], g["b2"], g["e"], g["weight_decay"], g["max_grad_norm"], float(CODES[type(sch).__name__]),
            float(sch.warmup), float(sch.t_total), float(getattr(sch, "cycles", 0.0)), 1.0,
            1.0 if g["bias_correction"] else 0.0, 1.0 if g["always_adapt"] else 0.0]


def table_of(groups, dev):
    rows = [row_of(g) for g in groups]
    assert all(len(r) == COLS for r in rows)
    return torch.tensor([x for r in rows for x in r], dtype=torch.float64).to(dev)


# The layout: sizes 1, 3, 5, 4096, 16384, 16385 and 40000 (one chunk, exactly one chunk, one element more, three chunks) and the
# special tensors.  Tensor 1 starts at arena offset 1 and tensor 5 at 20513: the scalar path of the norm (its first chunk; the
# second has length 1).  Groups: 0 decays (0.01), 1 does not, 2 does not but adapts always.
SIZES = [1, 3, 5, 4096, 16384, 16385, 40000, 64, 7, 4096, 300]
OFFSETS = [0, 1, 4, 12, 4108, 20513, 36900, 76900, 76964, 76972, 81068]
GID = [0, 1, 2, 0, 1, 2, 0, 1, 0, 0, 0]
SHADOWED = (3, 6)
PLAIN = 4                    # group 1: no decay, not always_adapt -> trust ratio 1 by rule
FROZEN, UNTOUCHED, ZERO_P, ZERO_G = 7, 8, 9, 10
START = [0, 3, 6, 9, 12, 15, 18, 5, 0, 2, 1]
N = len(SIZES)
LIVE = [i for i in range(N) if i not in (FROZEN, UNTOUCHED)]
assert all(OFFSETS[i] + SIZES[i] <= OFFSETS[i + 1] for i in range(N - 1)) and OFFSETS[5] % 4 == 1 and OFFSETS[6] % 4 == 0


def _groups(max_grad_norm=None):
    from visualbert_amd import optimization as opt
    gs = [dict(lr=1e-3, b1=0.9, b2=0.999, e=1e-6, weight_decay=0.01, max_grad_norm=1.0, bias_correction=True,
               always_adapt=False, schedule=opt.WarmupLinearSchedule(warmup=0.1, t_total=40)),
          dict(lr=2e-3, b1=0.8, b2=0.99, e=1e-8, weight_decay=0.0, max_grad_norm=0.5, bias_correction=False,
               always_adapt=False, schedule=opt.WarmupCosineSchedule(warmup=0.25, t_total=40, cycles=0.5)),
          dict(lr=5e-4, b1=0.85, b2=0.98, e=1e-5, weight_decay=0.0, max_grad_norm=2.0, bias_correction=True,
               always_adapt=True, schedule=opt.WarmupConstantSchedule(warmup=0.25, t_total=20))]
    if max_grad_norm is not None:
        for g in gs:
            g["max_grad_norm"] = max_grad_norm
    return gs


def _fresh(dev, seed=11, p_scale=None):
    """the arena in its starting state + the touched flags"""
    a = LambArena(dev, SIZES, OFFSETS, [(0 if i == FROZEN else 1) | (GID[i] << 2) for i in range(N)], SHADOWED)
    gen = torch.Generator().manual_seed(seed)
    p = torch.rand(a.params.numel(), generator=gen) * 2 - 1
    if p_scale:
        i, s = p_scale
        p[OFFSETS[i]:OFFSETS[i] + SIZES[i]] *= s
    a.params.copy_(p)
    a.view(a.params, ZERO_P).zero_()
    a.steps.copy_(torch.tensor(START, dtype=torch.int32))
    for b in (a.m, a.v):                                             # state a frozen tensor must keep
        a.view(b, FROZEN).copy_(torch.rand(SIZES[FROZEN], generator=gen))
    touched = torch.tensor([0.0 if i == UNTOUCHED else 1.0 for i in range(N)]).to(dev)
    return a, touched


def _gradients(launches, seed=12, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(launches):
        g = (torch.rand(OFFSETS[-1] + SIZES[-1], generator=gen) * 2 - 1) * scale
        for i in (UNTOUCHED, ZERO_G):
            g[OFFSETS[i]:OFFSETS[i] + SIZES[i]] = 0.0
        out.append(g)
    return out


def _restate(a0, grads, groups):
    """the restatement's run from the arena's starting state: {dtype: (P, M, V, S)}"""
    out = {}
    for dtype in (torch.float64, torch.float32):
        P = [a0.view(a0.params, i).cpu().to(dtype) for i in range(N)]
        M = [a0.view(a0.m, i).cpu().to(dtype) for i in range(N)]
        V = [a0.view(a0.v, i).cpu().to(dtype) for i in range(N)]
        S = list(START)
        for g in grads:
            G = [g[OFFSETS[i]:OFFSETS[i] + SIZES[i]] for i in range(N)]
            lamb_step(P, M, V, S, G, LIVE, GID, groups, dtype)
        out[dtype] = (P, M, V, S)
    return out


def _assert_within(a, ref, what=""):
    """asserts the bound of the module docstring per live tensor and buffer.  Measured worst excess (error over bound, 1 = at the
    bound) after the three launches of test_three_launches_match_the_restatement: params 0.21, exp_avg 0.25, exp_avg_sq 0.30 on
    MI355X (0.22, 0.25, 0.30 on the kernel-logic simulator); the worst of all tests that call this is exp_avg 0.31 (the one-element
    tensor in the edge-case run, on both)."""
    worst = {}
    for name, buf, k in (("params", a.params, 0), ("exp_avg", a.m, 1), ("exp_avg_sq", a.v, 2)):
        ex = [excess(a.view(buf, i), ref[torch.float32][k][i], ref[torch.float64][k][i]) for i in LIVE]
        worst[name] = max(ex)
        print("%s %s: worst excess %.3f (tensor %d)" % (what, name, max(ex), LIVE[ex.index(max(ex))]))
    for name, w in worst.items():
        assert w <= 1.0, (what, name, w)
    return worst


@pytest.fixture(scope="module")
def three_launch_reference(dev):
    """the restatement of the main case, computed once and only read by the tests that share it"""
    a0, _ = _fresh(dev)
    grads = _gradients(3)
    return grads, _restate(a0, grads, _groups())


@gpu
def test_three_launches_match_the_restatement(dev, three_launch_reference):
    grads, ref = three_launch_reference
    a, touched = _fresh(dev)
    frozen = [a.view(b, FROZEN).clone() for b in (a.params, a.m, a.v)]
    untouched = a.view(a.params, UNTOUCHED).clone()
    table = table_of(_groups(), dev)
    for launch, g in enumerate(grads):
        a.grads.copy_(g)
        assert a.step_lamb(table, 3, touched=touched, validate=1 if launch == 0 else 0) == 0
        assert torch.equal(a.grads.cpu(), g)                          # the gradient arena is only read
    _assert_within(a, ref, "three launches")
    for i in SHADOWED:
        o, n = OFFSETS[i], SIZES[i]
        assert torch.equal(a.shadow[o:o + n], a.params[o:o + n].to(torch.bfloat16))
    unshadowed = torch.ones(a.shadow.numel(), dtype=torch.bool)
    for i in SHADOWED:
        unshadowed[OFFSETS[i]:OFFSETS[i] + SIZES[i]] = False
    assert float(a.shadow.cpu()[unshadowed].float().abs().max()) == 0.0
    assert a.steps.cpu().tolist() == [s if i in (FROZEN, UNTOUCHED) else s + 3 for i, s in enumerate(START)]
    assert a.steps.cpu().tolist() == ref[torch.float64][3]
    for b, was in zip((a.params, a.m, a.v), frozen):                  # flag bit 0 clear: bit-unchanged
        assert torch.equal(a.view(b, FROZEN), was)
    assert torch.equal(a.view(a.params, UNTOUCHED), untouched)         # never touched, zero gradient, zero counter: no step
    assert float(a.view(a.m, UNTOUCHED).abs().max()) == 0.0 and float(a.view(a.v, UNTOUCHED).abs().max()) == 0.0
    # the tensor with a zero gradient and weight decay moved all the same (u = weight_decay * p, ratio 1 / weight_decay)
    assert float((a.view(a.params, ZERO_G).cpu() - ref[torch.float64][0][ZERO_G]).abs().max()) < 1e-6
    assert float(a.view(a.m, ZERO_G).abs().max()) == 0.0


@gpu
def test_trust_ratio_edge_cases(dev):
    groups = _groups()
    table = table_of(groups, dev)
    grads = _gradients(1, seed=21)
    runs = []
    for p_scale in (None, (PLAIN, 8.0)):
        a, touched = _fresh(dev, p_scale=p_scale)
        before = a.params.clone()
        ref = _restate(a, grads, groups)
        a.grads.copy_(grads[0])
        assert a.step_lamb(table, 3, touched=touched) == 0
        _assert_within(a, ref, "edge cases, ||p|| of tensor %d scaled: %s" % (PLAIN, p_scale is not None))
        runs.append((before, a.params.clone(), ref))
    before, after, ref = runs[0]
    # p == 0 everywhere: ||p|| = 0, so the ratio is 1 and the tensor moves by lr * schedule * u exactly
    o, n = OFFSETS[ZERO_P], SIZES[ZERO_P]
    h = groups[GID[ZERO_P]]
    assert float(before[o:o + n].abs().max()) == 0.0 and float(after[o:o + n].abs().min()) > 0.0
    g64 = grads[0][o:o + n].double()
    gn = float(torch.sqrt(sum((grads[0][OFFSETS[i]:OFFSETS[i] + SIZES[i]].double() ** 2).sum() for i in LIVE)))
    gc = g64 * min(1.0, h["max_grad_norm"] / (gn + 1e-6))
    t = START[ZERO_P] + 1
    m, v = (1 - h["b1"]) * gc / (1 - h["b1"] ** t), (1 - h["b2"]) * gc * gc / (1 - h["b2"] ** t)
    want = -h["lr"] * h["schedule"].get_lr(START[ZERO_P]) * (m / (v.sqrt() + h["e"]))            # ratio 1
    assert float((after[o:o + n].cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    # no decay, not always_adapt: ratio 1 whatever ||p|| -- with ||p|| scaled by 8 the tensor moves by the same lr * schedule * u
    # (each p - lr u is rounded at its own ulp(p): half an ulp of either scale; a ratio ||p|| / ||u|| would move it 8 x as far)
    o, n = OFFSETS[PLAIN], SIZES[PLAIN]
    d1 = (runs[0][1][o:o + n].double() - runs[0][0][o:o + n].double()).cpu()
    d8 = (runs[1][1][o:o + n].double() - runs[1][0][o:o + n].double()).cpu()
    assert float(d1.abs().max()) > 1e-4
    assert float((d8 - d1).abs().max()) <= 0.5 * (2.0 ** -23 + 2.0 ** -20)            # |p| < 2 and < 16 before and after


@gpu
def test_global_clipping(dev):
    """one norm over all groups: with max_grad_norm = 1 everywhere a gradient 100 times as large gives the clipped step of the
    unscaled one (whose norm is already far above 1); with max_grad_norm <= 0 the scale reaches the moments"""
    groups = _groups(max_grad_norm=1.0)
    grads = _gradients(1, seed=31)
    a0, _ = _fresh(dev)
    ref = _restate(a0, grads, groups)
    gn = float(torch.sqrt(sum((grads[0][OFFSETS[i]:OFFSETS[i] + SIZES[i]].double() ** 2).sum() for i in LIVE)))
    assert gn > 100.0
    for scale in (1.0, 100.0):
        a, touched = _fresh(dev)
        a.grads.copy_(grads[0] * scale)
        assert a.step_lamb(table_of(groups, dev), 3, touched=touched) == 0
        _assert_within(a, ref, "clipping, gradients x %g" % scale)
    # every group clips by the GLOBAL norm: a tensor of 3 elements had its moment scaled by 1 / gn, not by 1 / its own norm
    m1 = a0.view(a0.m, 1).cpu().double() * groups[1]["b1"] + (1 - groups[1]["b1"]) * grads[0][1:4].double() / (gn + 1e-6)
    assert float((a.view(a.m, 1).cpu().double() - m1).abs().max()) <= 1e-6 * float(m1.abs().max())
    unclipped = _groups(max_grad_norm=-1.0)
    ms = []
    for scale in (1.0, 100.0):
        a, touched = _fresh(dev)
        a.grads.copy_(grads[0] * scale)
        assert a.step_lamb(table_of(unclipped, dev), 3, touched=touched) == 0
        ms.append(a.view(a.m, 6).clone())
    assert float(ms[1].abs().max()) > 50.0 * float(ms[0].abs().max()) > 0.0


@gpu
def test_reduces_to_bert_adam_bit_for_bit(dev):
    """bias_correction = always_adapt = 0, no weight decay, no clipping: the same table (two columns shorter) through
    vb_bert_adam_step_groups gives the same bits"""
    groups = _groups(max_grad_norm=-1.0)
    for g in groups:
        g.update(weight_decay=0.0, bias_correction=False, always_adapt=False)
    grads = _gradients(3, seed=41)
    results = []
    for lamb in (True, False):
        a, touched = _fresh(dev)
        for g in grads:
            a.grads.copy_(g)
            if lamb:
                assert a.step_lamb(table_of(groups, dev), 3, touched=touched) == 0
            else:
                assert a.step_groups(adam_table_of([row_of(g_)[:11] for g_ in groups], dev), 3, touched=touched) == 0
        results.append(a.snapshot())
    for x, y in zip(*results):
        assert torch.equal(x, y)
    assert results[0][4].cpu().tolist() == [s if i in (FROZEN, UNTOUCHED) else s + 3 for i, s in enumerate(START)]
    assert not torch.equal(results[0][0], _fresh(dev)[0].params)


@gpu
def test_the_same_step_twice_gives_the_same_bits(dev):
    groups = _groups()
    a, touched = _fresh(dev)
    a.grads.copy_(_gradients(1, seed=51)[0])
    table = table_of(groups, dev)
    snap = a.snapshot()
    results = []
    for _ in range(2):
        a.restore(snap)
        a.ws.zero_()
        assert a.step_lamb(table, 3, touched=touched) == 0
        results.append(a.snapshot() + [a.ws.clone(), a.grads.clone()])
    for x, y in zip(*results):
        assert torch.equal(x, y)
    assert not a.unchanged_since(snap)


@gpu
def test_bad_tables_are_argument_errors_and_change_nothing(dev):
    groups = _groups()
    a, touched = _fresh(dev)
    a.grads.copy_(_gradients(1, seed=61)[0])
    snap = a.snapshot()
    good = table_of(groups, dev)
    assert a.step_lamb(None, 3) == VB_ERR_ARG                                         # no table
    assert a.step_lamb(good, 0) == VB_ERR_ARG                                         # no groups
    assert a.step_lamb(good, 2, touched=touched) == VB_ERR_ARG                        # tensors 2 and 5 name group 2
    rows = [row_of(g) for g in groups]
    rows[1][6] = 7.0
    bad = torch.tensor([x for r in rows for x in r], dtype=torch.float64).to(dev)
    assert a.step_lamb(bad, 3, touched=touched) == VB_ERR_ARG                         # unknown schedule code
    assert a.unchanged_since(snap)
    # validate = 0: the tensors of the bad group take no step (and give nothing to the global norm), the others do
    assert a.step_lamb(bad, 3, touched=touched, validate=0) == 0
    now = a.snapshot()
    for i in range(N):
        same = all(torch.equal(a.view(x, i), a.view(y, i)) for x, y in zip(snap[:3], now[:3]))
        assert same == (i in (FROZEN, UNTOUCHED) or GID[i] == 1), i
    assert now[4].cpu().tolist() == [s + (0 if (i in (FROZEN, UNTOUCHED) or GID[i] == 1) else 1) for i, s in enumerate(START)]
    a.restore(snap)
    assert a.step_lamb(good, 2, touched=touched, validate=0) == 0                     # group 2 is outside the table
    assert a.steps.cpu().tolist() == [s + (0 if (i in (FROZEN, UNTOUCHED) or GID[i] == 2) else 1) for i, s in enumerate(START)]


# ------------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------------
def _wrapper(dev, **extra):
    from visualbert_amd.model import ModelWrapper, AttrDict
    cfg, head, sd, batch, g = load_case("tiny_pretraining")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    args = AttrDict(train_batch_size=1, learning_rate=1e-3, warmup_proportion=0.1, num_train_epochs=1,
                    gradient_accumulation_steps=1, **extra)
    return ModelWrapper(args, T_TOTAL, model=model), model, to_dev(batch, dev)


@gpu
def test_wrapper_steps_follow_the_restatement(dev):
    """three steps of ModelWrapper with `optimizer: "lamb"`; the restatement is fed the gradients the kernels produced (read
    from the arena just before each optimizer step) and the two groups initialize_opimizer builds.
    Measured worst excess (error over bound) over all tensors on MI355X: params 0.17, exp_avg 0.23 - 0.33 (the backward pass
    accumulates some gradients with atomics, so runs differ), exp_avg_sq 0.25; on the kernel-logic simulator 0.18, 0.22, 0.25."""
    from visualbert_amd.optimization import Lamb
    mw, model, b = _wrapper(dev, optimizer="lamb")
    optim = mw.optimizer
    assert type(optim) is Lamb and len(optim.param_groups) == 2
    assert [g["weight_decay"] for g in optim.param_groups] == [0.01, 0.0]
    assert all(g["bias_correction"] is True and g["always_adapt"] is False and g["max_grad_norm"] == 1.0
               for g in optim.param_groups)
    arena = model.bert.arena
    names, params = arena.names, arena.params
    member = {id(p): gi for gi, g in enumerate(optim.param_groups) for p in g["params"]}
    assert all(("pooler" in n) == (id(p) not in member) for n, p in zip(names, params))
    groups = [dict(lr=g["lr"], b1=g["b1"], b2=g["b2"], e=g["e"], weight_decay=g["weight_decay"],
                   max_grad_norm=g["max_grad_norm"], schedule=g["schedule"], bias_correction=g["bias_correction"],
                   always_adapt=g["always_adapt"]) for g in optim.param_groups]
    gid = [member.get(id(p), 0) for p in params]
    n = len(params)
    state = {dt: ([p.detach().cpu().to(dt).reshape(-1) for p in params], [torch.zeros(p.numel(), dtype=dt) for p in params],
                  [torch.zeros(p.numel(), dtype=dt) for p in params], [0] * n) for dt in (torch.float64, torch.float32)}
    inner = optim.step
    seen = []

    def capturing_step():
        G = [p.grad.detach().cpu().reshape(-1).clone() for p in params]
        live = [i for i, p in enumerate(params) if id(p) in member and
                (id(p) in arena.touched or state[torch.float64][3][i] > 0 or float(G[i].abs().max()) > 0)]
        for dt in state:
            lamb_step(state[dt][0], state[dt][1], state[dt][2], state[dt][3], G, live, gid, groups, dt)
        seen.append(G)
        inner()
        assert all(torch.equal(p.grad.detach().cpu().reshape(-1), g0) for p, g0 in zip(params, G))     # .grad survives step()

    optim.step = capturing_step
    for _ in range(3):
        mw.step(b)
    assert len(seen) == 3
    sd = optim.state_dict()
    by_param = {id(p): sd["state"][k] for k, p in enumerate(p for g in optim.param_groups for p in g["params"])}
    worst = {"params": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for i, p in enumerate(params):
        if id(p) not in member:
            continue
        st = by_param[id(p)]
        assert st["step"] == state[torch.float64][3][i] == 3, names[i]
        for key, got, k in (("params", p.detach(), 0), ("exp_avg", st["exp_avg"], 1), ("exp_avg_sq", st["exp_avg_sq"], 2)):
            ex = excess(got, state[torch.float32][k][i], state[torch.float64][k][i])
            worst[key] = max(worst[key], ex)
            assert ex <= 1.0, (names[i], key, ex)
    print("wrapper, three steps: worst excess %s" % worst)
    for p in params:
        if p.dim() == 2 and id(p) in member:
            assert torch.equal(p._vb_shadow, p.detach().to(torch.bfloat16))
    assert optim.get_lr() == [g["lr"] * g["schedule"].get_lr(3) for g in (optim.param_groups[gid[i]] for i, p in
                                                                         enumerate(params) if id(p) in member)]
    assert optim.table_uploads == 1


@gpu
def test_checkpoint_resume_is_bit_identical(dev):
    """state_dict -> a fresh model and optimizer -> load_state_dict -> one more step on the same gradients: the parameters of the
    uninterrupted run, bit for bit"""
    mw, model, b = _wrapper(dev, optimizer="lamb", lamb_always_adapt=True)
    for _ in range(2):
        mw.step(b)
    buf = io.BytesIO()
    torch.save(copy.deepcopy(mw.state_dict()), buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    st = ck["optimizer"]["state"]
    assert set(st[0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and st[0]["step"] == 2
    assert all(isinstance(g["schedule"], dict) and g["always_adapt"] is True and g["bias_correction"] is True
               for g in ck["optimizer"]["param_groups"])
    mw2, model2, _ = _wrapper(dev, optimizer="lamb", lamb_bias_correction=False)      # configured differently: the checkpoint wins
    mw2.load_state_dict(ck)
    assert all(g["always_adapt"] is True and g["bias_correction"] is True for g in mw2.optimizer.param_groups)
    # one backward pass feeds both optimizers (the backward kernels accumulate some gradients with atomics, so two passes over
    # equal weights need not agree in the last bit; what is checked here is that the restored optimizer state is complete)
    arena, arena2 = model.bert.arena, model2.bert.arena
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    mw.optimizer.zero_grad()
    mw2.optimizer.zero_grad()
    model(**b)["loss"].backward()
    arena2.grad.copy_(arena.grad)
    arena2.touched = set(id(q) for p, q in zip(arena.params, arena2.params) if id(p) in arena.touched)
    assert len(arena2.touched) == len(arena.touched) > 0
    before = arena.data.clone()
    mw.optimizer.step()
    mw2.optimizer.step()
    assert not torch.equal(arena.data, before)
    for (n, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    member = set(id(p) for g in mw.optimizer.param_groups for p in g["params"])
    for p, q in zip(arena.params, arena2.params):                   # the bf16 copies the GEMMs read followed the step
        if p.dim() == 2 and id(p) in member:
            assert torch.equal(p._vb_shadow, q._vb_shadow) and torch.equal(p._vb_shadow, p.detach().to(torch.bfloat16))
    a, a2 = mw.optimizer.state_dict()["state"], mw2.optimizer.state_dict()["state"]
    assert all(a[k]["step"] == a2[k]["step"] == 3 and torch.equal(a[k]["exp_avg_sq"], a2[k]["exp_avg_sq"]) for k in a)


@gpu
def test_wrapper_default_is_still_bert_adam(dev):
    from visualbert_amd.optimization import BertAdam, Lamb
    mw, _, _ = _wrapper(dev)
    assert type(mw.optimizer) is BertAdam
    mw, _, _ = _wrapper(dev, optimizer="bert_adam")
    assert type(mw.optimizer) is BertAdam
    mw, _, _ = _wrapper(dev, optimizer="lamb", lamb_bias_correction=False, lamb_always_adapt=True)
    assert type(mw.optimizer) is Lamb
    assert all(g["bias_correction"] is False and g["always_adapt"] is True for g in mw.optimizer.param_groups)
    with pytest.raises(ValueError, match="optimizer"):
        _wrapper(dev, optimizer="adamw")


@gpu
def test_layerwise_groups_and_a_late_group(dev):
    """layerwise_groups feeds Lamb as it feeds BertAdam; a group added after a step joins with zero state, the others keep theirs"""
    from visualbert_amd.optimization import Lamb, layerwise_groups
    cfg, head, sd, batch, g = load_case("tiny_pretraining")
    model = build_model(cfg, head, sd, dev, dropout=0.0)
    model.train()
    named = list(model.named_parameters())
    groups = layerwise_groups(named, 1e-3, layer_decay=0.9, head_lr=4e-3)
    assert len(groups) > 2
    late = [gr for gr in groups if gr["lr"] == 4e-3]
    early = [gr for gr in groups if gr["lr"] != 4e-3]
    assert late and early
    optim = Lamb(early, lr=1e-3, warmup=0.1, t_total=T_TOTAL)
    b = to_dev(batch, dev)

    def one_step():
        optim.zero_grad()
        model(**b)["loss"].backward()
        optim.step()

    one_step()
    one_step()
    before = optim.state_dict()["state"]
    for gr in late:
        optim.add_param_group(gr)
    after = optim.state_dict()["state"]
    assert len(after) > len(before)
    for k in before:
        assert after[k]["step"] == before[k]["step"] == 2 and torch.equal(after[k]["exp_avg"], before[k]["exp_avg"])
    assert all(after[k]["step"] == 0 and float(after[k]["exp_avg_sq"].abs().max()) == 0.0 for k in after if k not in before)
    assert all(gr["bias_correction"] is True for gr in optim.param_groups)
    one_step()
    steps = [s["step"] for s in optim.state_dict()["state"].values()]
    assert steps == [3] * len(before) + [1] * (len(after) - len(before))
    assert len(set(optim.get_lr())) > 2
