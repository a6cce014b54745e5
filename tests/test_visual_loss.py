"""The masked-region objective (vb_visual_loss_fwd_bwd, ops.VisualLossFn, lxrt.BertVisualObjHead / LXRTPretrainingHeads) against the
restatement of the reference's loss lines in tests/visual_loss_restatement.py (fp64 = the reference, fp32 = the size of the bound).

fp32 bound: 4 x the fp32 restatement's own distance from the fp64 one on the same inputs (losses relative, gradient max-abs with an
absolute floor of 1e-7).  Measured on MI355X (profiles/visual_loss_parity.json, kernel error / bound over the seven shapes): see
MEASURED below -- the bound held as the issue states it, nothing was widened.  bf16: both sides start from the same bf16-rounded scores; losses meet the fp32 bound, every gradient element is within
one bf16 rounding of the fp64 value (2^-8 |ref|) plus the fp32 bound."""
import pytest
import torch

from golden_util import record
from visual_loss_restatement import bounds, loss_terms, visual_losses

pytestmark = pytest.mark.gpu

# (M; n_obj, n_attr, n_feat; ld)
CASES = [
    (72, 1600, 400, 2048, 4096),        # the real shape, B = 2 x 36
    (72, 1601, 401, 2048, 4096),        # vector path with segment boundaries inside a vector
    (5, 7, 5, 13, 25),                  # scalar path, unaligned pitch
    (1, 1600, 400, 2048, 4096),         # single row
    (300, 1600, 0, 0, 1600),            # one segment only; more rows than any slot or partial table
    (300, 0, 0, 2048, 2048),
    (300, 0, 400, 2048, 2448),          # one segment absent
]
W = (1 / 0.15, 5.0, 1 / 0.3)            # the reference's weight for obj; different ones for attr / feat so that a swap shows

#: kernel error over its bound (<= 1 passes), worst over CASES, as measured on MI355X (profiles/visual_loss_parity.json has every case).
#: fp32 losses: 0.25 means the kernel's loss IS the fp32 restatement's, bit for bit (five of seven cases); worst 0.66 (1601 | 401 | 2048).
#: fp32 gradient: worst 0.72 at M = 1 (bound 1.7e-6: the 1 / M scale is 1 there), <= 0.26 elsewhere (absolute floor 1e-7 in force).
#: bf16 gradient: 0.89 - 0.98 is the bf16 rounding itself (round-to-nearest errs by up to 2^-8 |ref|), not the arithmetic in front of it.
MEASURED = dict(fp32_loss=0.66, fp32_grad=0.72, bf16_loss=0.65, bf16_grad=0.98)


def make_inputs(M, n_obj, n_attr, n_feat, ld, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * seed + M + n_obj + 3 * n_attr + 7 * n_feat)
    scores = (torch.randn((M, ld), generator=g) * 3.0).to(dtype)

    def labels(n):
        lab = torch.randint(0, max(n, 1), (M,), generator=g, dtype=torch.int64)
        lab[torch.rand(M, generator=g) < 0.2] = -1
        lab[0] = min(3, max(n - 1, 0))
        return lab

    def conf():
        c = torch.rand(M, generator=g)
        c[torch.rand(M, generator=g) < 0.3] = 0.0
        c[0] = 0.7
        return c

    d = dict(M=M, n=(n_obj, n_attr, n_feat), ld=ld, scores=scores, obj_label=labels(n_obj), obj_conf=conf(),
             attr_label=labels(n_attr), attr_conf=conf())
    fm = (torch.rand(M, generator=g) < 0.15).float()
    fm[0] = 1.0                                             # row 0 always counts in every term: no loss is trivially 0
    d["feat_conf"] = fm
    e = torch.rand((M, n_feat), generator=g) * 6.0 - 3.0    # both SmoothL1 branches
    off = n_obj + n_attr
    d["feat_target"] = (scores[:, off:off + n_feat].float() - e).contiguous()
    return d


def restate(d, dtype, scores=None):
    n = d["n"]
    return visual_losses(d["scores"] if scores is None else scores, n[0], n[1], n[2], d["obj_label"], d["obj_conf"], d["attr_label"],
                         d["attr_conf"], d["feat_target"], d["feat_conf"], W[0], W[1], W[2], dtype=dtype)


def run_kernel(dev, d, mode="out", ld_d=None, scores=None, pad_fill=None, **over):
    """one call of the entry point.  mode: 'out' (separate dscores), 'alias' (dscores == scores), 'null' (no gradient).
    Returns (losses [4] on the CPU, dscores [M, ld_d] on the CPU or None)."""
    from visualbert_amd import _lib
    L = _lib.lib()
    M, (n_obj, n_attr, n_feat), ld = d["M"], d["n"], d["ld"]
    t = {k: over.get(k, d[k]).to(dev) for k in ("obj_label", "obj_conf", "attr_label", "attr_conf", "feat_target", "feat_conf")}
    s = (d["scores"] if scores is None else scores).clone().to(dev)
    ld_d = ld if (ld_d is None or mode == "alias") else ld_d
    out = None
    if mode == "out":
        out = torch.full((M, ld_d), float("nan") if pad_fill is None else pad_fill, dtype=s.dtype, device=dev)
    elif mode == "alias":
        out = s
    n_ws = L.vb_visual_loss_ws_floats(M)
    assert n_ws >= 3
    ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=dev)
    losses = torch.full((4,), float("nan"), dtype=torch.float32, device=dev)
    rc = L.vb_visual_loss_fwd_bwd(_lib.dtype_code(s.dtype), _lib.ptr(s), ld, n_obj, n_attr, n_feat,
                                  _lib.ptr(t["obj_label"]) if n_obj else None, _lib.ptr(t["obj_conf"]) if n_obj else None,
                                  _lib.ptr(t["attr_label"]) if n_attr else None, _lib.ptr(t["attr_conf"]) if n_attr else None,
                                  _lib.ptr(t["feat_target"]) if n_feat else None, n_feat,
                                  _lib.ptr(t["feat_conf"]) if n_feat else None, W[0], W[1], W[2], _lib.ptr(ws), _lib.ptr(losses),
                                  _lib.ptr(out), ld_d, M, _lib.stream_ptr())
    assert rc == 0, rc
    if dev.type == "cuda":
        torch.cuda.current_stream().synchronize()
    return losses.cpu(), (out.cpu() if out is not None else None)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def zero_bits(t):
    """every element is +0.0 (an empty tensor passes)"""
    return not bool((bits(t) != 0).any())


def loss_excess(got, l64, rel_bound):
    """worst (relative error / bound) over the four losses; a loss that is exactly 0 in fp64 must be exactly 0"""
    worst = 0.0
    for k in range(4):
        if float(l64[k]) == 0.0:
            assert float(got[k]) == 0.0, (k, float(got[k]))
            continue
        err = abs(float(got[k]) - float(l64[k])) / abs(float(l64[k]))
        worst = max(worst, err / max(float(rel_bound[k]), 1e-300))
    return worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_%d_%d_%d_ld%d" % c)
def test_fp32_kernel_against_the_fp64_restatement(dev, case):
    d = make_inputs(*case)
    r64, r32 = restate(d, torch.float64), restate(d, torch.float32)
    rel_bound, grad_bound = bounds(r32, r64)
    losses, ds = run_kernel(dev, d)
    width = sum(d["n"])
    gerr = float((ds[:, :width].double() - r64[1]).abs().max())
    lex = loss_excess(losses, r64[0], rel_bound)
    rec = dict(loss_err_over_bound=lex, grad_err=gerr, grad_bound=grad_bound, grad_err_over_bound=gerr / grad_bound,
               loss_rel_bound=[float(x) for x in rel_bound])
    record("fp32", "M%d_%d_%d_%d_ld%d" % case, rec, fname="visual_loss_parity.json")
    print("visual loss fp32 %s: %s" % (case, rec))
    assert torch.isfinite(losses).all() and torch.isfinite(ds[:, :width]).all()
    assert zero_bits(ds[:, width:])                           # pad columns: zero bits
    assert gerr <= grad_bound, rec
    assert lex <= 1.0, rec


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_%d_%d_%d_ld%d" % c)
def test_bf16_kernel_against_the_fp64_restatement(dev, case):
    d = make_inputs(*case, dtype=torch.bfloat16)
    sf = d["scores"].float()                                 # both sides start from the same bf16-rounded scores
    r64, r32 = restate(d, torch.float64, sf), restate(d, torch.float32, sf)
    rel_bound, grad_bound = bounds(r32, r64)
    losses, ds = run_kernel(dev, d)
    width = sum(d["n"])
    lex = loss_excess(losses, r64[0], rel_bound)
    err = (ds[:, :width].double() - r64[1]).abs()
    allowed = r64[1].abs() * 2.0 ** -8 + grad_bound
    gex = float((err / allowed).max())
    rec = dict(loss_err_over_bound=lex, grad_err_over_bound=gex)
    record("bf16", "M%d_%d_%d_%d_ld%d" % case, rec, fname="visual_loss_parity.json")
    print("visual loss bf16 %s: %s" % (case, rec))
    assert zero_bits(ds[:, width:])
    assert gex <= 1.0, rec
    assert lex <= 1.0, rec


SMALL = (40, 64, 24, 40, 192)                                # vector path, 64 pad columns, ten workgroups


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [SMALL, (11, 7, 5, 13, 27)], ids=["vector", "scalar"])
def test_ignored_work_is_exactly_ignored(dev, case, dtype):
    d = make_inputs(*case, seed=1, dtype=dtype)
    M, (n_obj, n_attr, n_feat) = d["M"], d["n"]
    losses, ds = run_kernel(dev, d)
    segs = ((0, n_obj, (d["obj_label"] < 0) | (d["obj_conf"] == 0)), (n_obj, n_attr, (d["attr_label"] < 0) | (d["attr_conf"] == 0)),
            (n_obj + n_attr, n_feat, d["feat_conf"] == 0))
    poisoned = d["scores"].clone()
    for off, n, ignored in segs:
        assert bool(ignored.any()) and not bool(ignored.all())
        assert zero_bits(ds[ignored][:, off:off + n])           # all-zero bits, not -0.0
        poisoned[ignored, off:off + n] = float("nan")
    # an ignored (row, segment) contributes exactly 0.0: whatever its scores hold -- NaN included -- the losses keep their bits
    losses_p, ds_p = run_kernel(dev, d, scores=poisoned)
    assert torch.equal(bits(losses), bits(losses_p)) and torch.equal(bits(ds), bits(ds_p))
    # labels >= n (and far beyond int32) behave as -1
    big = {}
    for key, n in (("obj_label", n_obj), ("attr_label", n_attr)):
        lab = d[key].clone()
        idx = torch.nonzero(lab < 0).reshape(-1)
        lab[idx] = torch.tensor([n, n + 5, 2 ** 40])[torch.arange(idx.numel()) % 3]
        big[key] = lab
    losses_b, ds_b = run_kernel(dev, d, **big)
    assert torch.equal(bits(losses), bits(losses_b)) and torch.equal(bits(ds), bits(ds_b))
    # every row ignored, each in its own way: four exact zeros (the mean is over M: no 0 / 0), an all-zero gradient
    none = dict(obj_label=torch.full((M,), -1, dtype=torch.int64), attr_conf=torch.zeros(M), feat_conf=torch.zeros(M))
    losses_0, ds_0 = run_kernel(dev, d, scores=torch.full_like(d["scores"], float("nan")), **none)
    assert torch.equal(losses_0, torch.zeros(4)) and zero_bits(losses_0)
    assert zero_bits(ds_0)


def test_smooth_l1_boundaries(dev):
    """e in {0, +-1, +-(1 - 2^-10), +-(1 + 2^-10)}: the restatement's branch and gradient.  With target 0, confidence 1 and
    w / (M n_feat) a power of two every product is exact, so the gradient must EQUAL the fp64 one."""
    h = 2.0 ** -10
    e = torch.tensor([0.0, 1.0, -1.0, 1.0 - h, -(1.0 - h), 1.0 + h, -(1.0 + h), 0.5])
    M, n_feat = 2, 8
    d = dict(M=M, n=(0, 0, n_feat), ld=n_feat, scores=torch.stack([e, -e.flip(0)]), feat_target=torch.zeros((M, n_feat)),
             feat_conf=torch.ones(M), obj_label=torch.zeros(M, dtype=torch.int64), obj_conf=torch.zeros(M),
             attr_label=torch.zeros(M, dtype=torch.int64), attr_conf=torch.zeros(M))
    global W
    old, W = W, (1.0, 1.0, 1.0)
    try:
        r64 = restate(d, torch.float64)
        losses, ds = run_kernel(dev, d)
    finally:
        W = old
    assert torch.equal(ds.double(), r64[1]), (ds, r64[1])
    assert abs(float(losses[2]) - float(r64[0][2])) <= 2.0 ** -22 * float(r64[0][2])       # a sum of 16 fp32 terms
    assert float(losses[3]) == float(losses[2]) and float(losses[0]) == 0.0 and float(losses[1]) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [SMALL, (6, 7, 5, 13, 29)], ids=["vector", "scalar"])
def test_extreme_logits_and_padding(dev, case, dtype):
    d = make_inputs(*case, seed=2, dtype=dtype)
    n_obj, n_attr, n_feat = d["n"]
    width = n_obj + n_attr + n_feat
    d["scores"][0, 0], d["scores"][0, 1], d["scores"][0, n_obj] = 80.0, -80.0, -80.0     # +-80 in one row (row 0 always counts)
    d["scores"][:, width:] = 0.0
    sf = d["scores"].float()
    r64, r32 = restate(d, torch.float64, sf), restate(d, torch.float32, sf)
    rel_bound, grad_bound = bounds(r32, r64)
    losses, ds = run_kernel(dev, d)
    assert torch.isfinite(losses).all() and torch.isfinite(ds.float()).all()
    # a handful of rows: the fp32 restatement can land on the correctly rounded loss by luck (a bound of 0), so the losses are held to
    # the number format instead -- 2^-21 relative, four fp32 roundings (the sum of exponentials, its log, lse - logit, the final cast)
    assert loss_excess(losses, r64[0], torch.full((4,), 2.0 ** -21, dtype=torch.float64)) <= 1.0
    allowed = (r64[1].abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0) + grad_bound
    assert bool(((ds[:, :width].double() - r64[1]).abs() <= allowed).all())
    # NaN in the padding columns of scores changes nothing; the padding columns of dscores come back as zeros, also when
    # dscores is wider than scores
    nan_pad = d["scores"].clone()
    nan_pad[:, width:] = float("nan")
    losses_n, ds_n = run_kernel(dev, d, scores=nan_pad)
    assert torch.equal(bits(losses), bits(losses_n)) and torch.equal(bits(ds), bits(ds_n))
    assert zero_bits(ds[:, width:])
    wide = d["ld"] + (64 if d["ld"] % 8 == 0 else 3)
    losses_w, ds_w = run_kernel(dev, d, ld_d=wide)
    assert torch.equal(bits(ds_w[:, :width]), bits(ds[:, :width])) and zero_bits(ds_w[:, width:])


def test_wide_gradient_pitch_is_zero_filled_past_the_register_span(dev):
    """ld_dscores beyond the 4096 columns a wave holds: the tail is zero-filled too (counted and ignored rows)"""
    d = make_inputs(6, 64, 24, 40, 128, seed=3)
    _, ds = run_kernel(dev, d, ld_d=4096 + 640)
    _, ref = run_kernel(dev, d)
    assert torch.equal(bits(ds[:, :128]), bits(ref)) and zero_bits(ds[:, 128:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["vector", "scalar"])
def test_aliasing_and_null_gradient(dev, case, dtype):
    d = make_inputs(*case, seed=4, dtype=dtype)
    losses, ds = run_kernel(dev, d, pad_fill=0.0)
    losses_a, ds_a = run_kernel(dev, d, mode="alias")
    losses_n, none = run_kernel(dev, d, mode="null")
    width = sum(d["n"])
    assert none is None
    assert torch.equal(bits(losses), bits(losses_a)) and torch.equal(bits(losses), bits(losses_n))
    assert torch.equal(bits(ds[:, :width]), bits(ds_a[:, :width]))
    assert zero_bits(ds_a[:, width:])


def test_argument_checks(dev):
    from visualbert_amd import _lib
    L = _lib.lib()
    assert L.vb_visual_loss_ws_floats(0) < 0 and L.vb_visual_loss_ws_floats(300) >= 900
    d = make_inputs(*SMALL)
    s = d["scores"].to(dev)
    p = _lib.ptr(s)
    lab, cf = _lib.ptr(d["obj_label"].to(dev)), _lib.ptr(d["obj_conf"].to(dev))
    sp = _lib.stream_ptr()
    # too narrow a pitch, a missing label, a row wider than a wave holds: refused before any launch
    assert L.vb_visual_loss_fwd_bwd(0, p, 100, 64, 24, 40, lab, cf, lab, cf, p, 40, cf, 1.0, 1.0, 1.0, p, p, None, 0, 40, sp) == _lib.VB_ERR_ARG
    assert L.vb_visual_loss_fwd_bwd(0, p, 192, 64, 24, 0, None, cf, lab, cf, None, 0, None, 1.0, 1.0, 1.0, p, p, None, 0, 40, sp) == _lib.VB_ERR_ARG
    assert L.vb_visual_loss_fwd_bwd(0, p, 8192, 4000, 24, 80, lab, cf, lab, cf, p, 80, cf, 1.0, 1.0, 1.0, p, p, None, 0, 1, sp) == _lib.VB_ERR_UNSUPPORTED


def test_losses_repeat_bit_for_bit(dev):
    d = make_inputs(*CASES[6], seed=5)
    first, _ = run_kernel(dev, d, mode="null")
    again, _ = run_kernel(dev, d, mode="null")
    assert torch.equal(bits(first), bits(again))
    if dev.type == "cuda":
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            other, ds_other = run_kernel(dev, d)
        torch.cuda.synchronize()
        assert torch.equal(bits(first), bits(other))
        _, ds = run_kernel(dev, d)
        assert torch.equal(bits(ds), bits(ds_other))


# ---- module level: H = 128 (2 heads of 64), M = 2 x 36 regions --------------------------------------------------------------
H, B, R = 128, 2, 36
SIZES = {"obj": 104, "attr": 40, "feat": 72}                 # multiples of 8, none of 64: ragged GEMM tiles, ld = 256
#: bf16: max loss error and worst per-tensor gradient relative L2, 1.5 x the values measured on MI355X (profiles/visual_loss_parity.json:
#: 1.37e-2 at |loss| <= 48 -- the feature term of a head with N(0, 0.3) weights -- and 7.94e-3, decoder_dict.feat.weight)
BF16_BOUNDS = dict(loss=2.06e-2, grad_worst=1.19e-2)


def head_case(seed=7):
    from visualbert_amd import lxrt
    from visualbert_amd.modeling import BertConfig
    torch.manual_seed(seed)
    bc = BertConfig(96, hidden_size=H, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    head = lxrt.BertVisualObjHead(bc, "obj,attr,feat", sizes=SIZES)
    for p in head.parameters():
        p.data.normal_(0.0, 0.3)
    head.transform.LayerNorm.weight.data.add_(1.0)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, R, H), generator=g)
    M = B * R
    lab = dict(obj=torch.randint(0, SIZES["obj"], (B, R), generator=g), attr=torch.randint(0, SIZES["attr"], (B, R), generator=g))
    lab["obj"][0, :7] = -1
    lab["attr"][1, 3:9] = -1
    conf = dict(obj=torch.rand((B, R), generator=g), attr=torch.rand((B, R), generator=g),
                feat=(torch.rand((B, R), generator=g) < 0.3).float())
    conf["obj"][1, :5] = 0.0
    target = torch.randn((B, R, SIZES["feat"]), generator=g) * 2.0
    return bc, head, x, lab, conf, target, M


def head_reference(head, x, lab, conf, target):
    """the same head with torch.nn.functional on the CPU in fp64, from the same state dict"""
    import torch.nn.functional as F
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in head.state_dict().items()}
    xin = x.double().clone().requires_grad_(True)
    h = F.gelu(F.linear(xin.reshape(-1, H), sd["transform.dense.weight"], sd["transform.dense.bias"]))
    h = F.layer_norm(h, (H,), sd["transform.LayerNorm.weight"], sd["transform.LayerNorm.bias"], eps=1e-12)
    sc = torch.cat([F.linear(h, sd["decoder_dict.%s.weight" % k], sd["decoder_dict.%s.bias" % k]) for k in ("obj", "attr", "feat")], 1)
    terms = loss_terms(sc, SIZES["obj"], SIZES["attr"], SIZES["feat"], lab["obj"], conf["obj"], lab["attr"], conf["attr"],
                       target, conf["feat"], W[0], W[1], W[2])
    # a weighted sum, so that a per-term upstream scalar that went missing shows
    total = 1.0 * terms[0] + 0.5 * terms[1] + 2.0 * terms[2]
    total.backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads["visn_output"] = xin.grad
    return torch.stack([t.detach() for t in terms]), grads


def head_run(dev, mode):
    from visualbert_amd import ops
    bc, head, x, lab, conf, target, M = head_case()
    ref_losses, ref_grads = head_reference(head, x, lab, conf, target)
    head = head.to(dev)
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    xin = x.to(dev).to(dt).requires_grad_(True)
    with ops.x3_scope(mode == "bf16x3"):
        scores = head(xin)
        assert scores.dtype == dt and scores.shape[0] == M and scores.stride(0) % 64 == 0
        losses = ops.VisualLossFn.apply(scores, SIZES["obj"], SIZES["attr"], SIZES["feat"], lab["obj"].to(dev), conf["obj"].to(dev),
                                        lab["attr"].to(dev), conf["attr"].to(dev), target.to(dev), conf["feat"].to(dev), *W)
        total = 1.0 * losses[0] + 0.5 * losses[1] + 2.0 * losses[2]
    total.backward()
    got = {k: p.grad.detach().double().cpu() for k, p in head.named_parameters()}
    got["visn_output"] = xin.grad.detach().double().cpu()
    loss_err = float((losses.detach().double().cpu() - ref_losses).abs().max())
    rels = {k: float((got[k] - ref_grads[k]).norm()) / float(ref_grads[k].norm()) for k in ref_grads}
    return loss_err, rels, float(ref_losses.abs().max())


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_head_and_loss_match_the_fp64_head(dev, mode):
    loss_err, rels, loss_max = head_run(dev, mode)
    worst = max(rels, key=rels.get)
    rec = dict(loss_err=loss_err, loss_absmax=loss_max, grad_rel_l2_worst=rels[worst], grad_rel_l2_worst_name=worst)
    record("head_" + mode, "H128_M72", rec, fname="visual_loss_parity.json")
    print("visual head %s: %s" % (mode, rec))
    if mode == "bf16":
        assert loss_err <= BF16_BOUNDS["loss"] and rels[worst] <= BF16_BOUNDS["grad_worst"], rec
    else:                                                    # the bounds of tests/test_lxrt.py's fp32 test
        assert loss_err < 1e-4, rec
        assert rels[worst] <= 2e-3, rec


def heads_case(dev):
    from visualbert_amd import lxrt
    bc, head, x, lab, conf, target, M = head_case(seed=9)
    torch.manual_seed(9)
    emb = torch.nn.Parameter(torch.randn(96, H) * 0.05)
    heads = lxrt.LXRTPretrainingHeads(bc, emb, sizes=SIZES)
    heads.apply(lxrt.lxrt_init_weights)
    heads.obj_predict_head.load_state_dict(head.state_dict())
    heads = heads.to(dev)
    g = torch.Generator().manual_seed(9)
    T = 12
    lang = torch.randn((B, T, H), generator=g).to(dev)
    pooled = torch.randn((B, H), generator=g).to(dev)
    mlm = torch.randint(0, 96, (B, T), generator=g)
    mlm[torch.rand((B, T), generator=g) < 0.7] = -1
    mlm[0, 1] = 5
    obj_labels = {"obj": (lab["obj"].to(dev), conf["obj"].to(dev)), "attr": (lab["attr"].to(dev), conf["attr"].to(dev)),
                  "feat": (target.to(dev), conf["feat"].to(dev))}
    return heads, emb, lang, pooled, x.to(dev), mlm.to(dev), torch.tensor([1, 0]).to(dev), obj_labels


def test_pretraining_heads_end_to_end(dev):
    heads, emb, lang, pooled, visn, mlm, matched, obj_labels = heads_case(dev)
    lang, pooled, visn = lang.requires_grad_(True), pooled.requires_grad_(True), visn.requires_grad_(True)
    total, losses, losses_dict = heads(lang, pooled, visn, masked_lm_labels=mlm, matched_label=matched, obj_labels=obj_labels)
    assert list(losses_dict.keys()) == ["Masked LM", "Matches", "obj", "attr", "feat"]       # the reference's order and names
    assert losses.shape == (1, 5) and not losses.requires_grad
    for i, k in enumerate(losses_dict):
        assert float(losses[0, i]) == float(losses_dict[k]) and float(losses_dict[k]) > 0.0
    parts = losses[0, 0]
    for i in range(1, 5):
        parts = parts + losses[0, i]
    assert float(total) == float(parts)                       # the sum of its parts, added in the reference's order
    total.backward()
    for name, p in list(heads.named_parameters()) + [("lang", lang), ("pooled", pooled), ("visn", visn)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, name
    # a subset of the visual losses in another order: the terms follow visual_losses, the values are those of the full head
    from visualbert_amd import lxrt
    from visualbert_amd.modeling import BertConfig
    bc = BertConfig(96, hidden_size=H, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    sub = lxrt.LXRTPretrainingHeads(bc, emb, task_mask_lm=False, task_matched=False, visual_losses="feat,obj", sizes=SIZES,
                                    loss_weight=1.0).to(dev)
    full = heads.obj_predict_head.state_dict()
    sub.obj_predict_head.load_state_dict({k: v for k, v in full.items() if "decoder_dict.attr" not in k})
    with torch.no_grad():
        total_s, losses_s, dict_s = sub(None, None, visn, obj_labels=obj_labels)
    assert list(dict_s.keys()) == ["feat", "obj"] and losses_s.shape == (1, 2)
    w = 1 / 0.15
    assert abs(float(dict_s["feat"]) * w - float(losses_dict["feat"])) <= 1e-5 * float(losses_dict["feat"])
    assert abs(float(dict_s["obj"]) * w - float(losses_dict["obj"])) <= 1e-5 * float(losses_dict["obj"])


def test_no_grad_writes_no_gradient(dev):
    from visualbert_amd import ops
    heads, emb, lang, pooled, visn, mlm, matched, obj_labels = heads_case(dev)
    head = heads.obj_predict_head
    args = [SIZES["obj"], SIZES["attr"], SIZES["feat"], obj_labels["obj"][0], obj_labels["obj"][1], obj_labels["attr"][0],
            obj_labels["attr"][1], obj_labels["feat"][0], obj_labels["feat"][1], 1.0, 1.0, 1.0]
    with torch.no_grad():
        scores = head(visn)
        keep = scores.clone()
        losses = ops.VisualLossFn.apply(scores, *args)
        assert torch.equal(bits(scores), bits(keep))          # dscores was NULL: the score buffer still holds the scores
        total, _, _ = heads(lang, pooled, visn, masked_lm_labels=mlm, matched_label=matched, obj_labels=obj_labels)
    assert not losses.requires_grad and not total.requires_grad
    assert all(p.grad is None for p in heads.parameters())
    scores = head(visn)                                       # with autograd on, the same call leaves the gradient in the buffer
    losses_g = ops.VisualLossFn.apply(scores, *args)
    assert torch.equal(bits(losses_g.detach()), bits(losses))
    width = sum(SIZES.values())
    assert not torch.equal(bits(scores.detach()[:, :width]), bits(keep[:, :width]))
    # a consumer that is not the head's decoder node receives the gradient scaled by the upstream scalars
    leaf = keep.clone().requires_grad_(True)
    la = ops.VisualLossFn.apply(leaf * 1.0, *args)
    (3.0 * la[3]).backward()
    ref = restate_scores(keep, obj_labels)
    assert float((leaf.grad[:, :width].double().cpu() - 3.0 * ref).abs().max()) <= 3.0 * 1e-6


def restate_scores(scores, obj_labels):
    _, g = visual_losses(scores.float(), SIZES["obj"], SIZES["attr"], SIZES["feat"], obj_labels["obj"][0], obj_labels["obj"][1],
                         obj_labels["attr"][0], obj_labels["attr"][1], obj_labels["feat"][0], obj_labels["feat"][1], 1.0, 1.0, 1.0)
    return g
