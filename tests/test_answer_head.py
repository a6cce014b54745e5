"""The answer head of the sibling LXRT model on the HIP kernels -- vb_ln_wide_fwd / vb_ln_wide_bwd (GELU + LayerNorm over wide rows),
vb_bce_logits_fwd_bwd (the VQA fine-tuning loss), lxrt.BertVisualAnswerHead, lxrt.LXRTPretrainingHeadsQA -- against the restatement of
the reference's lines in tests/answer_head_restatement.py (fp64 = the reference, fp32 = the size of the bound).

fp32 bound, per output: max-abs error against fp64 <= 4 x the fp32 restatement's own max-abs distance from fp64 on the same inputs,
with the floor 1e-7 x max|reference|.  bf16: both sides start from the same bf16-rounded inputs; every element of y / dx is within one
bf16 rounding of the fp64 value (2^-8 |ref|) plus the fp32 bound, the fp32 accumulators dgamma / dbeta meet the fp32 bound.
BCE loss: relative error <= max(4 x the restatement's, 2^-23 ceil(log2(M V))).  Measured on MI355X: MEASURED below
(profiles/answer_head_parity.json has every case)."""
import pytest
import torch

import answer_head_restatement as R
from golden_util import record

pytestmark = pytest.mark.gpu

PARITY = "answer_head_parity.json"
GELU, NONE = 1, 0                                            # VB_ACT_GELU / VB_ACT_NONE

# (M, H, act)
LN_CASES = [
    (32, 1536, GELU),        # the real shape
    (3, 1032, GELU),         # first width past the narrow kernels' limit, ragged second pass
    (1, 2048, GELU),         # exactly one full pass, single row
    (5, 2056, NONE),         # one lane in the second pass
    (300, 1536, GELU),       # more rows than workgroups or partial slots
    (2, 8192, GELU),         # the maximum width
    (4, 8, GELU),            # one chunk
    (32, 1536, NONE),        # the real shape without GELU
]
# (M, V, ld)
BCE_CASES = [(32, 3129, 3136), (1, 3129, 3136), (5, 7, 9), (300, 1842, 1848)]

#: kernel error over its bound (<= 1 passes), worst over the cases, as measured on MI355X
#: fp32 LayerNorm: worst 0.47 (dbeta at M = 4, H = 8); y / dx / dgamma <= 0.34 on every shape.
#: bf16 y / dx: 0.99 is the bf16 rounding itself (round-to-nearest errs by up to 2^-8 |ref| just above a power of two).
#: BCE: the loss sits at 0.003 - 0.03 of its bound (fp64 tree over fp32 row terms), score equal on all four shapes.
MEASURED = dict(ln_fp32=dict(y=0.34, dx=0.26, dgamma=0.25, dbeta=0.47), ln_bf16=dict(y=0.995, dx=0.996, dgamma=0.48, dbeta=0.25),
                bce=dict(loss=0.03, grad=0.24))


def ln_id(c):
    return "M%d_H%d_%s" % (c[0], c[1], "gelu" if c[2] else "none")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.current_stream().synchronize()


def guarded(M, H, dtype, dev):
    """[M + 2, H] filled with NaN: the kernel gets the first M rows, the last two must stay as they are"""
    return torch.full((M + 2, H) if H else (M + 2,), float("nan"), dtype=dtype, device=dev)


def untouched(t, M):
    return bool(torch.isnan(t[M:].float()).all())


def run_ln(dev, x, dy, gamma, beta, act, dtype=torch.float32, alias=False, dg0=None, db0=None, want=("dgamma", "dbeta")):
    """one forward and one backward call on their own buffers.  Returns dict(y, mean, rstd, dx, dgamma, dbeta) on the CPU."""
    from visualbert_amd import _lib
    L = _lib.lib()
    M, H = x.shape
    code = _lib.dtype_code(dtype)
    xd, gd, bd = x.to(dtype).to(dev), gamma.to(dev), beta.to(dev)
    y, mean, rstd = guarded(M, H, dtype, dev), guarded(M, 0, torch.float32, dev), guarded(M, 0, torch.float32, dev)
    rc = L.vb_ln_wide_fwd(code, _lib.ptr(xd), act, _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gd), _lib.ptr(bd), M, H,
                          R.EPS, _lib.stream_ptr())
    assert rc == 0, rc
    sync(dev)
    assert untouched(y, M) and untouched(mean, M) and untouched(rstd, M)
    n_ws = L.vb_ln_wide_bwd_ws_floats(M, H)
    assert n_ws >= 2 * H
    ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=dev)
    dyd = guarded(M, H, dtype, dev)
    dyd[:M] = dy.to(dtype).to(dev)
    dx = dyd if alias else guarded(M, H, dtype, dev)
    dg = (torch.zeros(H) if dg0 is None else dg0.clone()).to(dev)
    db = (torch.zeros(H) if db0 is None else db0.clone()).to(dev)
    rc = L.vb_ln_wide_bwd(code, _lib.ptr(dyd), _lib.ptr(xd), act, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gd), _lib.ptr(dx),
                          _lib.ptr(dg) if "dgamma" in want else None, _lib.ptr(db) if "dbeta" in want else None, _lib.ptr(ws),
                          M, H, _lib.stream_ptr())
    assert rc == 0, rc
    sync(dev)
    assert untouched(dx, M) and untouched(dyd, M)
    return dict(y=y[:M].cpu(), mean=mean[:M].cpu(), rstd=rstd[:M].cpu(), dx=dx[:M].cpu(), dgamma=dg.cpu(), dbeta=db.cpu())


@pytest.mark.parametrize("case", LN_CASES, ids=ln_id)
def test_ln_fp32_against_the_fp64_restatement(dev, case):
    M, H, act = case
    x, dy, gamma, beta = R.ln_inputs(M, H)
    r64, r32 = R.ln_case(x, dy, gamma, beta, act, torch.float64), R.ln_case(x, dy, gamma, beta, act, torch.float32)
    got = run_ln(dev, x, dy, gamma, beta, act)
    rec = {}
    for k in ("y", "dx", "dgamma", "dbeta"):
        b = R.bound(r32[k], r64[k])
        err = float((got[k].double() - r64[k]).abs().max())
        rec[k] = dict(err=err, bound=b, err_over_bound=err / b)
    record("ln_fp32", ln_id(case), rec, fname=PARITY)
    print("wide LN fp32 %s: %s" % (ln_id(case), rec))
    assert all(bool(torch.isfinite(got[k]).all()) for k in got)
    for k, v in rec.items():
        assert v["err"] <= v["bound"], (k, rec)


@pytest.mark.parametrize("case", LN_CASES, ids=ln_id)
def test_ln_bf16_against_the_fp64_restatement(dev, case):
    M, H, act = case
    x, dy, gamma, beta = R.ln_inputs(M, H)
    xb, dyb = x.bfloat16().float(), dy.bfloat16().float()     # both sides start from the same bf16-rounded x / dy
    r64, r32 = R.ln_case(xb, dyb, gamma, beta, act, torch.float64), R.ln_case(xb, dyb, gamma, beta, act, torch.float32)
    got = run_ln(dev, xb, dyb, gamma, beta, act, dtype=torch.bfloat16)
    rec = {}
    for k in ("y", "dx"):
        allowed = r64[k].abs() * 2.0 ** -8 + R.bound(r32[k], r64[k])
        rec[k] = dict(err_over_bound=float(((got[k].double() - r64[k]).abs() / allowed).max()))
    for k in ("dgamma", "dbeta"):
        b = R.bound(r32[k], r64[k])
        err = float((got[k].double() - r64[k]).abs().max())
        rec[k] = dict(err=err, bound=b, err_over_bound=err / b)
    record("ln_bf16", ln_id(case), rec, fname=PARITY)
    print("wide LN bf16 %s: %s" % (ln_id(case), rec))
    for k, v in rec.items():
        assert v["err_over_bound"] <= 1.0, (k, rec)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [LN_CASES[1], LN_CASES[4]], ids=ln_id)
def test_ln_backward_contracts(dev, case, dtype):
    """accumulation onto prior contents, NULL dgamma / dbeta, dx over dy, repeatability; ws starts as NaN and the guard rows behind
    every output stay NaN in each call (run_ln)"""
    M, H, act = case
    x, dy, gamma, beta = R.ln_inputs(M, H, seed=1)
    base = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype)
    again = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype)
    for k in base:
        assert torch.equal(bits(base[k]), bits(again[k])), k  # two calls, the same bits
    g = torch.Generator().manual_seed(5)
    dg0, db0 = torch.randn(H, generator=g) * 3.0, torch.randn(H, generator=g) * 3.0
    acc = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype, dg0=dg0, db0=db0)
    assert torch.equal(acc["dgamma"], dg0 + base["dgamma"]) and torch.equal(acc["dbeta"], db0 + base["dbeta"])
    only_g = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype, dg0=dg0, db0=db0, want=("dgamma",))
    assert torch.equal(bits(only_g["dgamma"]), bits(acc["dgamma"])) and torch.equal(only_g["dbeta"], db0)
    only_b = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype, dg0=dg0, db0=db0, want=("dbeta",))
    assert torch.equal(bits(only_b["dbeta"]), bits(acc["dbeta"])) and torch.equal(only_b["dgamma"], dg0)
    neither = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype, dg0=dg0, db0=db0, want=())
    assert torch.equal(neither["dgamma"], dg0) and torch.equal(neither["dbeta"], db0)
    assert torch.equal(bits(neither["dx"]), bits(base["dx"]))
    alias = run_ln(dev, x, dy, gamma, beta, act, dtype=dtype, alias=True)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(bits(alias[k]), bits(base[k])), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ln_constant_row_gives_beta(dev, dtype):
    """a row of all 0.5 without GELU: the mean is exact, the variance 0, rstd = 1 / sqrt(eps) -- y == beta exactly, all finite"""
    M, H = 3, 1536
    x, dy, gamma, beta = R.ln_inputs(M, H, seed=2)
    x[1] = 0.5
    got = run_ln(dev, x, dy, gamma, beta, NONE, dtype=dtype)
    assert all(bool(torch.isfinite(got[k].float()).all()) for k in got)
    assert float(got["mean"][1]) == 0.5
    assert torch.equal(got["y"][1], beta.to(dtype))


def test_ln_argument_checks(dev):
    from visualbert_amd import _lib
    L = _lib.lib()
    assert L.vb_ln_wide_bwd_ws_floats(32, 1536) >= 2 * 1536 and L.vb_ln_wide_bwd_ws_floats(300, 8) >= 16
    for M, H in ((32, 1540), (32, 8200), (0, 1536), (32, 0)):
        assert L.vb_ln_wide_bwd_ws_floats(M, H) < 0
    t = torch.full((4, 8200), float("nan"), dtype=torch.float32, device=dev)
    p, sp = _lib.ptr(t), _lib.stream_ptr()
    # H not a multiple of 8, H beyond 8192, no rows, an activation the kernel does not have, a missing pointer: refused, nothing launched
    for M, H, act in ((2, 1540, GELU), (2, 8200, GELU), (0, 1536, GELU), (2, 1536, 7)):
        assert L.vb_ln_wide_fwd(0, p, act, p, p, p, p, p, M, H, 1e-12, sp) == _lib.VB_ERR_ARG
        assert L.vb_ln_wide_bwd(0, p, p, act, p, p, p, p, p, p, p, M, H, sp) == _lib.VB_ERR_ARG
    assert L.vb_ln_wide_fwd(0, p, GELU, None, p, p, p, p, 2, 1536, 1e-12, sp) == _lib.VB_ERR_ARG
    assert L.vb_ln_wide_bwd(0, p, p, GELU, p, p, p, p, p, p, None, 2, 1536, sp) == _lib.VB_ERR_ARG      # ws is required
    assert L.vb_ln_wide_fwd(5, p, GELU, p, p, p, p, p, 2, 1536, 1e-12, sp) == _lib.VB_ERR_ARG           # no such dtype
    sync(dev)
    assert bool(torch.isnan(t).all())


# ---- BCE ------------------------------------------------------------------------------------------------------------------------
def run_bce(dev, logits, target, ld, mode="out", ld_t=None, want_score=True):
    """one call.  mode 'out': dlogits [M, ld] over a NaN pre-fill; 'null': no gradient.  Returns (loss, score, dlogits) on the CPU."""
    from visualbert_amd import _lib
    L = _lib.lib()
    M, V = logits.shape
    lg = torch.full((M, ld), float("nan"), dtype=torch.float32)      # NaN in the pad columns of the logits: never looked at
    lg[:, :V] = logits
    ld_t = V if ld_t is None else ld_t
    tg = torch.full((M, ld_t), float("nan"), dtype=torch.float32)
    tg[:, :V] = target
    lg, tg = lg.to(dev), tg.to(dev)
    n_ws = L.vb_bce_logits_ws_floats(M)
    assert n_ws >= 2 * M
    ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    score = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    out = torch.full((M + 2, ld), float("nan"), dtype=torch.float32, device=dev) if mode == "out" else None
    rc = L.vb_bce_logits_fwd_bwd(_lib.ptr(lg), ld, _lib.ptr(tg), ld_t, _lib.ptr(ws), _lib.ptr(loss),
                                 _lib.ptr(score) if want_score else None, _lib.ptr(out), ld, M, V, _lib.stream_ptr())
    assert rc == 0, rc
    sync(dev)
    if out is not None:
        assert untouched(out, M)
        out = out[:M].cpu()
    return loss.cpu(), score.cpu(), out


def bce_id(c):
    return "M%d_V%d_ld%d" % c


@pytest.mark.parametrize("case", BCE_CASES, ids=bce_id)
def test_bce_against_the_fp64_restatement(dev, case):
    M, V, ld = case
    logits, target = R.bce_inputs(M, V)
    assert R.unique_argmax(logits) and float(logits.max()) == 90.0 and float(logits.min()) == -90.0
    assert float(target[M - 1].abs().sum()) == 0.0 and float(target.min()) >= 0.0 and float(target.max()) <= 1.0
    (l64, g64, s64), (l32, g32, s32) = R.bce_case(logits, target, torch.float64), R.bce_case(logits, target, torch.float32)
    loss, score, dl = run_bce(dev, logits, target, ld)
    gb = R.bound(g32, g64)
    gerr = float((dl[:, :V].double() - g64).abs().max())
    lb = R.loss_rel_bound(l32, l64, M, V)
    lerr = abs(float(loss) - float(l64)) / abs(float(l64))
    rec = dict(loss_rel_err=lerr, loss_rel_bound=lb, loss_err_over_bound=lerr / lb, grad_err=gerr, grad_bound=gb,
               grad_err_over_bound=gerr / gb, score=float(score.detach()))
    record("bce", bce_id(case), rec, fname=PARITY)
    print("bce %s: %s" % (bce_id(case), rec))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
    assert not bool((bits(dl[:, V:]) != 0).any())             # pad columns: zero bits over the NaN pre-fill
    assert gerr <= gb, rec
    assert lerr <= lb, rec
    assert float(score) == float(s64.float()), (float(score), float(s64))
    if M > 1:
        assert float(score) > 0.0
    # no gradient wanted, no score wanted, a padded target pitch, a second call: the same loss bits
    loss_n, score_n, none = run_bce(dev, logits, target, ld, mode="null")
    loss_s, _, dl_s = run_bce(dev, logits, target, ld, want_score=False)
    loss_t, score_t, dl_t = run_bce(dev, logits, target, ld, ld_t=ld)
    loss_2, score_2, dl_2 = run_bce(dev, logits, target, ld)
    assert none is None
    for other in (loss_n, loss_s, loss_t, loss_2):
        assert torch.equal(bits(loss), bits(other))
    for other in (score_n, score_t, score_2):
        assert torch.equal(bits(score), bits(other))
    for other in (dl_s, dl_t, dl_2):
        assert torch.equal(bits(dl), bits(other))


def test_bce_argument_checks(dev):
    from visualbert_amd import _lib
    L = _lib.lib()
    assert L.vb_bce_logits_ws_floats(0) < 0 and L.vb_bce_logits_ws_floats(300) >= 600
    t = torch.full((4, 16), float("nan"), dtype=torch.float32, device=dev)
    p, sp = _lib.ptr(t), _lib.stream_ptr()
    assert L.vb_bce_logits_fwd_bwd(p, 8, p, 16, p, p, None, None, 0, 4, 9, sp) == _lib.VB_ERR_ARG        # pitch below V
    assert L.vb_bce_logits_fwd_bwd(p, 16, p, 16, p, p, None, p, 8, 4, 9, sp) == _lib.VB_ERR_ARG          # gradient pitch below V
    assert L.vb_bce_logits_fwd_bwd(p, 16, p, 16, None, p, None, None, 0, 4, 9, sp) == _lib.VB_ERR_ARG    # ws is required
    assert L.vb_bce_logits_fwd_bwd(p, 16, p, 16, p, p, None, None, 0, 0, 9, sp) == _lib.VB_ERR_ARG
    sync(dev)
    assert bool(torch.isnan(t).all())


# ---- modules --------------------------------------------------------------------------------------------------------------------
B = 8
HEAD_SHAPES = {"base": (768, 3129), "micro": (64, 37)}       # (H, num_answers)
#: fp32 / bf16x3: error over the 4 x rule's bound, measured on MI355X, for the quantities where the GEMMs' own error breaks the rule at
#: module level (the kernels of this head alone sit at <= 0.47 of it, MEASURED above): the fp32 GEMMs chain K = 768 / 1536 / 3129
#: products in one accumulator where the CPU restatement's GEMMs add blocked partial sums, and bf16x3 drops the lo x lo product
#: (~2^-16 relative per product).  Those quantities are asserted at 2 x the measured error (README: bounds of this kind); every
#: quantity not listed here -- all of the micro head in fp32, both losses -- is held to the rule itself.
HEAD_RATIO_MEASURED = {
    ("base", "fp32"): {"logits": 1.01, "grad logit_fc.0.weight": 1.28, "grad logit_fc.0.bias": 1.43, "grad logit_fc.2.weight": 1.38},
    ("micro", "fp32"): {},
    ("base", "bf16x3"): {"logits": 4.41, "grad logit_fc.0.weight": 6.49, "grad logit_fc.0.bias": 5.13, "grad logit_fc.2.weight": 3.82,
                         "grad logit_fc.2.bias": 3.29, "grad logit_fc.3.weight": 4.22, "grad logit_fc.3.bias": 3.26, "grad pooled": 2.85},
    ("micro", "bf16x3"): {"logits": 5.54, "grad logit_fc.0.weight": 6.80, "grad logit_fc.0.bias": 3.51, "grad logit_fc.2.weight": 1.38,
                          "grad logit_fc.2.bias": 3.61, "grad logit_fc.3.weight": 6.45, "grad logit_fc.3.bias": 2.89, "grad pooled": 4.41},
}
#: bf16: max-abs error against the fp64 restatement, measured on MI355X (profiles/answer_head_parity.json); asserted at 1.5 x.
#: base: |logits| <= 9, loss ~ 2.2e3 (a sum over 3129 answers); micro: 37 answers.
HEAD_BF16_MEASURED = {
    "base": {"logits": 3.11e-2, "loss": 1.28e-1, "grad logit_fc.0.weight": 2.50e-2, "grad logit_fc.0.bias": 2.53e-2,
             "grad logit_fc.2.weight": 4.03e-2, "grad logit_fc.2.bias": 1.22e-2, "grad logit_fc.3.weight": 9.11e-3,
             "grad logit_fc.3.bias": 2.03e-3, "grad pooled": 1.15e-2},
    "micro": {"logits": 4.56e-3, "loss": 7.42e-4, "grad logit_fc.0.weight": 2.77e-3, "grad logit_fc.0.bias": 4.22e-3,
              "grad logit_fc.2.weight": 8.81e-4, "grad logit_fc.2.bias": 7.65e-4, "grad logit_fc.3.weight": 3.32e-3,
              "grad logit_fc.3.bias": 7.93e-4, "grad pooled": 6.98e-4},
}


def head_setup(name, dev, dtype):
    from visualbert_amd import lxrt
    from visualbert_amd.modeling import BertConfig
    H, A = HEAD_SHAPES[name]
    bc = BertConfig(96, hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64, intermediate_size=4 * H)
    sd = R.head_state(H, A)
    head = lxrt.BertVisualAnswerHead(bc, A)
    head.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(11)
    pooled = torch.tanh(torch.randn((B, H), generator=g))
    if dtype == torch.bfloat16:
        pooled = pooled.bfloat16().float()                   # both sides start from the same bf16-rounded input
    logits0 = R.head_logits(sd, pooled)
    target = torch.zeros((B, A))
    label = logits0.argmax(1)
    for r in range(B - 1):                                    # the last row stays all zero
        target[r, label[r] if r % 2 == 0 else (5 * r + 1) % A] = R.SOFT_SCORES[r % 4]
        target[r, (7 * r + 3) % A] = 0.3
    return sd, head.to(dev), pooled, target


def head_run(dev, name, mode):
    from visualbert_amd import ops
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    sd, head, pooled, target = head_setup(name, dev, dt)
    xin = pooled.to(dev).to(dt).requires_grad_(True)
    with ops.x3_scope(mode == "bf16x3"):
        plain = head(xin.detach())
        logits, loss, score = head(xin, target=target.to(dev))
    assert plain.dtype == torch.float32 and logits.dtype == torch.float32 and not logits.requires_grad
    assert torch.equal(plain, logits)
    loss.backward()
    got = dict(logits=logits.detach().double().cpu(), loss=loss.detach().double().cpu(), score=float(score.detach()))
    got["grads"] = {k: p.grad.detach().double().cpu() for k, p in head.named_parameters()}
    got["grads"]["pooled"] = xin.grad.detach().double().cpu()
    return got, sd, pooled, target


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["base", "micro"])
def test_answer_head_fp32_against_the_fp64_restatement(dev, name, mode):
    got, sd, pooled, target = head_run(dev, name, mode)
    r64, r32 = R.head_case(sd, pooled, torch.float64, target=target), R.head_case(sd, pooled, torch.float32, target=target)
    ratios = {"logits": float((got["logits"] - r64["logits"]).abs().max()) / R.bound(r32["logits"], r64["logits"]),
              "loss": abs(float(got["loss"]) - float(r64["loss"])) / R.bound(r32["loss"], r64["loss"])}
    for k, g in r64["grads"].items():
        ratios["grad " + k] = float((got["grads"][k] - g).abs().max()) / R.bound(r32["grads"][k], g)
    worst = max(ratios, key=ratios.get)
    rec = dict(err_over_rule=ratios, worst=worst, worst_ratio=ratios[worst])
    record("head_" + mode, name, rec, fname=PARITY)
    print("answer head %s %s: %s" % (name, mode, rec))
    assert got["score"] == float(r64["score"].float())
    measured = HEAD_RATIO_MEASURED[(name, mode)]
    for k, ratio in ratios.items():
        assert ratio <= max(1.0, 2.0 * measured.get(k, 0.0)), (k, rec)


@pytest.mark.parametrize("name", ["base", "micro"])
def test_answer_head_bf16_against_the_fp64_restatement(dev, name):
    got, sd, pooled, target = head_run(dev, name, "bf16")
    r64 = R.head_case(sd, pooled, torch.float64, target=target)
    errs = {"logits": float((got["logits"] - r64["logits"]).abs().max()), "loss": abs(float(got["loss"]) - float(r64["loss"]))}
    for k, g in r64["grads"].items():
        errs["grad " + k] = float((got["grads"][k] - g).abs().max())
    record("head_bf16", name, errs, fname=PARITY)
    print("answer head %s bf16: %s" % (name, errs))
    measured = HEAD_BF16_MEASURED[name]
    for k, e in errs.items():
        assert e <= 1.5 * measured[k], (k, e, measured[k])


QA_H, QA_ANSWERS, QA_R, QA_T = 768, 9500, 36, 12
QA_SIZES = {"obj": 104, "attr": 40, "feat": 72}


def test_pretraining_heads_with_the_qa_term(dev):
    from visualbert_amd import lxrt
    from visualbert_amd.modeling import BertConfig
    torch.manual_seed(13)
    bc = BertConfig(96, hidden_size=QA_H, num_hidden_layers=1, num_attention_heads=12, intermediate_size=3072)
    emb = torch.nn.Parameter(torch.randn(96, QA_H) * 0.05)
    heads = lxrt.LXRTPretrainingHeadsQA(bc, emb, QA_ANSWERS, sizes=QA_SIZES)
    heads.apply(lxrt.lxrt_init_weights)
    sd = R.head_state(QA_H, QA_ANSWERS, seed=1)
    heads.answer_head.load_state_dict(sd, strict=True)
    heads = heads.to(dev)
    g = torch.Generator().manual_seed(13)
    lang = torch.randn((B, QA_T, QA_H), generator=g).to(dev).requires_grad_(True)
    pooled_cpu = torch.tanh(torch.randn((B, QA_H), generator=g))
    pooled = pooled_cpu.to(dev).requires_grad_(True)
    visn = torch.randn((B, QA_R, QA_H), generator=g).to(dev).requires_grad_(True)
    mlm = torch.randint(0, 96, (B, QA_T), generator=g)
    mlm[torch.rand((B, QA_T), generator=g) < 0.7] = -1
    mlm[0, 1] = 5
    matched = torch.randint(0, 2, (B,), generator=g)
    obj_labels = {"obj": (torch.randint(0, QA_SIZES["obj"], (B, QA_R), generator=g).to(dev), torch.rand((B, QA_R), generator=g).to(dev)),
                  "attr": (torch.randint(0, QA_SIZES["attr"], (B, QA_R), generator=g).to(dev), torch.rand((B, QA_R), generator=g).to(dev)),
                  "feat": (torch.randn((B, QA_R, QA_SIZES["feat"]), generator=g).to(dev),
                           (torch.rand((B, QA_R), generator=g) < 0.3).float().to(dev))}
    ans = torch.randint(0, QA_ANSWERS, (B,), generator=g)
    ans[1], ans[4], ans[B - 1] = -1, -1, -1                    # more than half of the pre-training data has no answer label
    assert int((ans >= 0).sum()) >= 1
    total, losses, answer_score, losses_dict = heads(lang, pooled, visn, masked_lm_labels=mlm.to(dev), matched_label=matched.to(dev),
                                                     obj_labels=obj_labels, ans=ans.to(dev))
    assert list(losses_dict.keys()) == ["Masked LM", "Matches", "obj", "attr", "feat", "qa"]    # the reference's order and names
    assert losses.shape == (1, 6) and not losses.requires_grad
    for i, k in enumerate(losses_dict):
        assert float(losses[0, i]) == float(losses_dict[k]) and float(losses_dict[k]) > 0.0
    parts = losses[0, 0]
    for i in range(1, 6):
        parts = parts + losses[0, i]
    assert float(total.detach()) == float(parts)              # the sum of its parts, added in the reference's order
    assert not answer_score.requires_grad and answer_score.shape == (B, QA_ANSWERS) and answer_score.dtype == torch.float32
    with torch.no_grad():
        assert torch.equal(answer_score, heads.answer_head(pooled))
    # the qa term and the answer scores against the restatement (fp32 kernels: the 4 x rule's floor is far below; 1e-4 as the fp32
    # head tests of tests/test_visual_loss.py)
    r64 = R.head_case(sd, pooled_cpu, torch.float64, labels=ans)
    assert float((answer_score.double().cpu() - r64["logits"]).abs().max()) < 1e-4
    assert abs(float(losses_dict["qa"]) - float(r64["loss"])) < 1e-4
    total.backward()
    for name, p in list(heads.named_parameters()) + [("lang", lang), ("pooled", pooled), ("visn", visn)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, name
    for k in R.HEAD_KEYS:
        got = heads.answer_head.state_dict(keep_vars=True)[k].grad.double().cpu()
        want = r64["grads"][k]
        assert float((got - want).norm()) <= 2e-3 * float(want.norm()), k
    # without ans the head still runs (the reference's constant return signature) and no term is added
    with torch.no_grad():
        total_n, losses_n, score_n, dict_n = heads(lang, pooled, visn, masked_lm_labels=mlm.to(dev), matched_label=matched.to(dev),
                                                   obj_labels=obj_labels)
    assert list(dict_n.keys()) == ["Masked LM", "Matches", "obj", "attr", "feat"] and torch.equal(score_n, answer_score)
