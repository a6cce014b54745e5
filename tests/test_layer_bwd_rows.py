"""vb_bert_layer_bwd_rows: the backward of the LAST encoder layer over the rows that carry a gradient, against the dense entry.

The contract under test: d_out is zero outside `rows`, and under that promise the rows entry computes what vb_bert_layer_bwd computes.
Both entries run from the same saved state of one forward (H = 768, I = 3072, 12 heads -- what the layer kernels are built for -- at
B x S = 3 x 23: S % 16 != 0, B S = 69 is no multiple of 64; and 12 x 23 = 276 rows, where "all rows" pads to two 256-row tiles).

Yardstick at p = 0: an fp32 torch restatement of the layer (autograd through it) on the same inputs.  The dense entry's own error
against it is measured per output -- d_in and the 16 parameter gradients (q / k / v taken apart) -- as max |got - ref|, and the rows
entry may miss the restatement by at most 1.5 x that: its weight-gradient and column sums add fewer terms in another order and a
compact GEMM may take another kernel (split-K at that M); the arithmetic is otherwise the same.  At p = 0.1 (hidden and attention
dropout) there is no restatement of the masks, so rows is held against dense directly: max |rows - dense| <= 1.5 x the dense error
measured at p = 0 for the same shape and row set.  A dropout mask replayed from the compact row number instead of the original one
misses that by orders of magnitude.  The empty set must give exact zeros (the bound is 0).

Measured on MI355X (worst over the 17 outputs; bound 1.5): every p = 0 case has ratio 1.000 (both entries miss the restatement by
the same 2.0e-3 ... 1.3e-2: at these sizes the compact GEMMs give a row the same result as the dense ones), every p = 0.1 case has
|rows - dense| <= 2.4e-7 against dense errors of 5.9e-5 ... 1.3e-2 (ratio <= 0.0006; the differences are the column sums' order),
the empty set gives exact zeros, and the model-level step has ratio 1.000 on all 50 parameters.  The kernel-logic simulator gives the
same picture.  Every run prints its own figures per output before it asserts.
"""
import ctypes

import pytest
import torch

from visualbert_amd import _lib

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H, I, NH = 768, 3072, 12
SHAPES = {"69": (3, 23), "276": (12, 23)}
MARGIN = 1.5
NAMES = ["d_in", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "g1", "b1", "wi", "bi", "wo2", "bo2", "g2", "b2"]


def _row_set(kind, B, S, dev):
    M = B * S
    g = torch.Generator(device="cpu").manual_seed(11)
    cls = torch.arange(B) * S
    if kind == "cls":
        r = cls
    elif kind == "random12":
        pick = torch.randperm(M, generator=g)[:max(1, int(round(0.12 * M)))]
        r = torch.unique(torch.cat((pick, cls)))
    elif kind == "single":
        r = torch.tensor([S + 7])
    elif kind == "all":
        r = torch.arange(M)
    elif kind == "empty":
        r = torch.empty(0, dtype=torch.int64)
    else:
        raise KeyError(kind)
    return torch.sort(r.to(torch.int64)).values.to(dev)


def _ptr_array(items):
    arr = (ctypes.c_void_p * len(items))()
    for i, t in enumerate(items):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


_STATE = {}                                     # (shape, p) -> problem + saved forward state, made once
_DENSE_ERR = {}                                 # (shape, row set) -> {output: dense error against the fp32 restatement at p = 0}


def _problem(shape, dev):
    B, S = SHAPES[shape]
    M = B * S
    g = torch.Generator(device="cpu").manual_seed(5)

    def rn(*s, scale=1.0, dt=torch.float32):
        return (torch.randn(*s, generator=g) * scale).to(dt).to(dev)

    P = dict(h_in=rn(M, H, dt=BF), wqkv=rn(3 * H, H, scale=0.04, dt=BF), bqkv=rn(3 * H, scale=0.1), wo=rn(H, H, scale=0.04, dt=BF),
             bo=rn(H, scale=0.1), g1=1.0 + rn(H, scale=0.1), b1=rn(H, scale=0.1), wi=rn(I, H, scale=0.04, dt=BF), bi=rn(I, scale=0.1),
             wo2=rn(H, I, scale=0.02, dt=BF), bo2=rn(H, scale=0.1), g2=1.0 + rn(H, scale=0.1), b2=rn(H, scale=0.1))
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    lens[-1] = S
    P["mask_add"] = ((torch.arange(S)[None, :] >= lens[:, None]).float() * -10000.0).contiguous().to(dev)
    for k in ("wqkv", "wo", "wi", "wo2"):
        P[k + "_t"] = P[k].t().contiguous()
    return P


def _state(shape, p, dev):
    key = (shape, p)
    st = _STATE.get(key)
    if st is not None:
        return st
    B, S = SHAPES[shape]
    M = B * S
    P = _STATE[(shape, "P")] = _STATE.get((shape, "P")) or _problem(shape, dev)
    L = _lib.lib()
    code = _lib.VB_BF16
    saved = torch.empty(L.vb_bert_layer_saved_bytes(code, B, S, H, I, NH, float(p)), dtype=torch.uint8, device=dev)
    scratch = torch.empty(L.vb_bert_layer_scratch_bytes(code, B, S, H, I, NH), dtype=torch.uint8, device=dev)
    h_out = torch.empty(M, H, dtype=BF, device=dev)
    weights = [P["wqkv"], P["bqkv"], P["wo"], P["bo"], P["g1"], P["b1"], P["wi"], P["bi"], P["wo2"], P["bo2"], P["g2"], P["b2"]]
    _lib.check(L.vb_bert_layer_fwd(code, _lib.ptr(P["h_in"]), _lib.ptr(P["mask_add"]), _lib.ptr(h_out), _lib.ptr(saved), _lib.ptr(scratch),
                                   _ptr_array(weights), B, S, H, I, NH, float(p), float(p), 1e-12, 0x1234567, 40, _lib.stream_ptr()),
               "vb_bert_layer_fwd")
    st = _STATE[key] = dict(P=P, saved=saved, h_out=h_out, weights=weights)
    return st


def _d_out(shape, kind, rows, dev):
    B, S = SHAPES[shape]
    g = torch.Generator(device="cpu").manual_seed(23)
    d = torch.zeros(B * S, H, dtype=BF, device=dev)
    if rows.numel():
        d[rows] = (torch.randn(rows.numel(), H, generator=g) * 0.05).to(BF).to(dev)
    return d


def _backward(shape, p, st, d_out, rows, dev):
    """the 17 outputs of one backward call: the dense entry (rows is None) or the rows entry"""
    B, S = SHAPES[shape]
    M = B * S
    P = st["P"]
    L = _lib.lib()
    code = _lib.VB_BF16
    masters = [P["wqkv"], P["bqkv"], P["wo"], P["bo"], P["g1"], P["b1"], P["wi"], P["bi"], P["wo2"], P["bo2"], P["g2"], P["b2"]]
    grads = [torch.zeros(w.shape, dtype=torch.float32, device=dev) for w in masters]
    d_in = torch.full((M, H), float("nan"), dtype=BF, device=dev)
    wts = [P["wqkv_t"], P["wo_t"], P["wi_t"], P["wo2_t"]]
    ld_t = (ctypes.c_int64 * 4)(*[w.stride(0) for w in wts])
    head = (code, _lib.ptr(P["h_in"]), _lib.ptr(st["h_out"]), _lib.ptr(P["mask_add"]), _lib.ptr(d_out), _lib.ptr(d_in), _lib.ptr(st["saved"]))
    tail = (_ptr_array(st["weights"]), _ptr_array(grads), _ptr_array(wts), ld_t, B, S, H, I, NH, float(p), float(p), 0x1234567, 40)
    if rows is None:
        scratch = torch.empty(L.vb_bert_layer_scratch_bytes(code, B, S, H, I, NH), dtype=torch.uint8, device=dev)
        _lib.check(L.vb_bert_layer_bwd(*head, _lib.ptr(scratch), *tail, _lib.stream_ptr()), "vb_bert_layer_bwd")
    else:
        n = int(rows.numel())
        nscr = L.vb_bert_layer_bwd_rows_scratch_bytes(code, B, S, H, I, NH, n)
        assert nscr > 0
        scratch = torch.empty(nscr, dtype=torch.uint8, device=dev)
        _lib.check(L.vb_bert_layer_bwd_rows(*head, _lib.ptr(scratch), *tail, _lib.ptr(rows) if n else None, n, _lib.stream_ptr()),
                   "vb_bert_layer_bwd_rows")
    gw, gb = grads[0].view(3, H, H), grads[1].view(3, H)
    outs = [d_in.float(), gw[0], gb[0], gw[1], gb[1], gw[2], gb[2]] + grads[2:]
    return dict(zip(NAMES, outs))


def _ln(z, gamma, beta):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return gamma * (z - mean) / torch.sqrt(var + 1e-12) + beta


def _restatement(shape, st, d_out):
    """fp32 torch restatement of the layer (pytorch_pretrained_bert/modeling.py:331-341, erf GELU, p = 0); autograd gives the 17 outputs"""
    B, S = SHAPES[shape]
    P = st["P"]
    leaves = {k: P[k].float().clone().requires_grad_(True) for k in
              ("h_in", "wqkv", "bqkv", "wo", "bo", "g1", "b1", "wi", "bi", "wo2", "bo2", "g2", "b2")}
    h = leaves["h_in"]
    qkv = (h @ leaves["wqkv"].t() + leaves["bqkv"]).view(B, S, 3, NH, 64).permute(2, 0, 3, 1, 4)
    sc = qkv[0] @ qkv[1].transpose(-1, -2) / 8.0 + P["mask_add"][:, None, None, :]
    ctx = (torch.softmax(sc, -1) @ qkv[2]).permute(0, 2, 1, 3).reshape(B * S, H)
    a_out = _ln(ctx @ leaves["wo"].t() + leaves["bo"] + h, leaves["g1"], leaves["b1"])
    inter = torch.nn.functional.gelu(a_out @ leaves["wi"].t() + leaves["bi"])
    out = _ln(inter @ leaves["wo2"].t() + leaves["bo2"] + a_out, leaves["g2"], leaves["b2"])
    out.backward(d_out.float())
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    gw, gb = g["wqkv"].view(3, H, H), g["bqkv"].view(3, H)
    outs = [g["h_in"], gw[0], gb[0], gw[1], gb[1], gw[2], gb[2]] + [g[k] for k in ("wo", "bo", "g1", "b1", "wi", "bi", "wo2", "bo2", "g2", "b2")]
    return dict(zip(NAMES, outs))


def _err(a, b):
    return float((a.float() - b.float()).abs().max())


def _dense_err(shape, kind, dev):
    """the dense entry's error against the restatement at p = 0, per output (measured once per shape and row set), + both results"""
    key = (shape, kind)
    if key not in _DENSE_ERR:
        st = _state(shape, 0.0, dev)
        rows = _row_set(kind, *SHAPES[shape], dev)
        d_out = _d_out(shape, kind, rows, dev)
        dense = _backward(shape, 0.0, st, d_out, None, dev)
        ref = _restatement(shape, st, d_out)
        _DENSE_ERR[key] = ({k: _err(dense[k], ref[k]) for k in NAMES}, ref)
    return _DENSE_ERR[key]


def _report(tag, figures):
    """print every figure before anything is asserted"""
    worst = max(figures.values(), key=lambda f: f[0] / f[1] if f[1] > 0 else (0.0 if f[0] == 0 else float("inf")))
    line = "%s: " % tag + "  ".join("%s %.3g/%.3g" % (k, f[0], f[1]) for k, f in figures.items())
    print(line)
    print("%s: worst ratio %.3f" % (tag, worst[0] / worst[1] if worst[1] > 0 else (0.0 if worst[0] == 0 else float("inf"))))


CASES = [("69", k) for k in ("cls", "random12", "single", "all", "empty")] + [("276", "random12"), ("276", "all")]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape,kind", CASES)
def test_rows_entry_against_dense_entry(dev, shape, kind, p):
    B, S = SHAPES[shape]
    rows = _row_set(kind, B, S, dev)
    d_out = _d_out(shape, kind, rows, dev)
    dense_err, ref = _dense_err(shape, kind, dev)
    st = _state(shape, p, dev)
    got = _backward(shape, p, st, d_out, rows, dev)
    if p == 0.0:
        figures = {k: (_err(got[k], ref[k]), dense_err[k]) for k in NAMES}          # rows error, dense error: both against the restatement
    else:
        dense = _backward(shape, p, st, d_out, None, dev)
        figures = {k: (_err(got[k], dense[k]), dense_err[k]) for k in NAMES}        # |rows - dense|, dense error at p = 0
    _report("B*S=%s rows=%s (%d) p=%.1f" % (shape, kind, rows.numel(), p), figures)
    for k in NAMES:
        assert torch.isfinite(got[k]).all(), k
        e, bound = figures[k]
        assert e <= MARGIN * bound, "%s: %.4g > %.1f x %.4g" % (k, e, MARGIN, bound)


def test_rows_entry_declines_what_it_does_not_cover(dev):
    """fp32 (and the split-operand mode) stay with the dense entry: VB_ERR_UNSUPPORTED, nothing launched"""
    L = _lib.lib()
    assert L.vb_bert_layer_bwd_rows_scratch_bytes(_lib.VB_F32, 3, 23, H, I, NH, 5) < 0
    x = torch.zeros(16, dtype=torch.float32, device=dev)
    p = _lib.ptr(x)
    arr12 = (ctypes.c_void_p * 12)(*[x.data_ptr()] * 12)
    arr4 = (ctypes.c_void_p * 4)(*[x.data_ptr()] * 4)
    ld = (ctypes.c_int64 * 4)(H, H, H, H)
    for code in (_lib.VB_F32, _lib.VB_BF16X3):
        rc = L.vb_bert_layer_bwd_rows(code, p, p, p, p, p, p, p, arr12, arr12, arr4, ld, 3, 23, H, I, NH, 0.0, 0.0, 1, 1, p, 1, None)
        assert rc == -3, rc


def test_row_check_kernel(dev):
    L = _lib.lib()
    M = 70
    rows = torch.tensor([0, 23, 46, 50], dtype=torch.int64, device=dev)
    x = torch.zeros(M, H, dtype=BF, device=dev)
    x[rows] = 1.0
    bad = torch.empty(2, dtype=torch.int32, device=dev)

    def run(xx, rr):
        _lib.check(L.vb_rows_check(_lib.VB_BF16, _lib.ptr(xx), _lib.ptr(rr), int(rr.numel()), M, H, _lib.ptr(bad), _lib.stream_ptr()), "vb_rows_check")
        return bad.tolist()

    assert run(x, rows) == [0, 0]
    y = x.clone()
    y[M - 1, H - 1] = -0.0                          # a negative zero is a zero
    assert run(y, rows) == [0, 0]
    y[M - 1, H - 1] = 1e-30
    assert run(y, rows) == [1, 0]
    assert run(x, torch.tensor([0, 46, 23, 50], dtype=torch.int64, device=dev))[1] == 1
    assert run(x, torch.tensor([0, 23, 23, 46, 50], dtype=torch.int64, device=dev))[1] == 1


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _tiny_step(dev, rows_on, plant=False, head="pretraining"):
    from oracle import visualbert_oracle as vo
    from visualbert_amd import ops
    from visualbert_amd.modeling import BertConfig
    from visualbert_amd.model import VisualBERTFixedImageEmbedding
    cfg = vo.OracleConfig(**vo.CONFIGS["micro"])
    sd = vo.synth_state_dict(cfg, head, 0)
    batch = vo.synth_batch(cfg, 3, 23, 6, 0, head)
    bc = BertConfig(cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                    num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = VisualBERTFixedImageEmbedding(config=bc, training_head_type=head, visual_embedding_dim=cfg.visual_embedding_dim,
                                          compute_dtype=BF).to(dev)
    own = model.bert.state_dict()
    with torch.no_grad():
        for k, v in sd.items():
            own[k].copy_(v)
    model.train()
    old = ops.set_grad_rows(rows_on)
    seen = []
    hook = model.bert.bert.encoder.layer[-1].register_forward_hook(lambda m, i, o: seen.append(o))
    try:
        taken = ops.grad_rows_taken()
        out = model(**{k: v.to(dev) for k, v in batch.items()})
        loss = out["loss"]
        if plant:                                   # one more consumer of the last layer's output, outside the declared rows:
            lab = batch["masked_lm_labels"]         # an unlabelled text position (not [CLS]) of the second sample
            t = int(torch.nonzero(lab[1, 1:] == -1)[0]) + 1
            S_all = seen[0].size(1)
            loss = loss + seen[0].reshape(-1, cfg.hidden_size)[S_all + t].float().sum()
        loss.backward()
        taken = ops.grad_rows_taken() - taken
    finally:
        hook.remove()
        ops.set_grad_rows(old)
    grads = {n: p.grad.detach().float().cpu().clone() for n, p in model.bert.named_parameters() if p.grad is not None}
    return cfg, sd, batch, out, grads, taken


def test_pretraining_step_with_and_without_the_rows_path(dev):
    """one step of a small pre-training model with the switch on and off: the forward is untouched (loss and logits bit-identical), the
    last layer's backward took the rows entry exactly once, and every parameter's gradient -- what the optimizer turns into the
    update -- misses the fp32 oracle by at most 1.5 x what the dense path misses it by"""
    from oracle import visualbert_oracle as vo
    cfg, sd, batch, out_on, g_on, taken_on = _tiny_step(dev, True)
    _, _, _, out_off, g_off, taken_off = _tiny_step(dev, False)
    assert (taken_on, taken_off) == (1, 0)
    assert torch.equal(out_on["loss"], out_off["loss"])
    assert torch.equal(out_on["logits"], out_off["logits"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    vo.objective_forward(leaves, cfg, "pretraining", mode="fp32", **batch)["loss"].backward()
    figures = {}
    for n in sorted(g_off):
        if leaves[n].grad is None:
            continue
        figures[n] = (_err(g_on[n], leaves[n].grad), _err(g_off[n], leaves[n].grad))
    _report("pre-training step, gradients", figures)
    assert len(figures) > 30
    for n, (e, bound) in figures.items():
        assert e <= MARGIN * bound, "%s: %.4g > %.1f x %.4g" % (n, e, MARGIN, bound)


def test_debug_check_raises_on_a_gradient_outside_the_rows(dev):
    from visualbert_amd import ops
    old = ops.set_grad_rows_check(True)
    try:
        _tiny_step(dev, True)                                   # the model's own heads keep the promise
        with pytest.raises(RuntimeError, match="not zero outside the rows"):
            _tiny_step(dev, True, plant=True)
    finally:
        ops.set_grad_rows_check(old)
