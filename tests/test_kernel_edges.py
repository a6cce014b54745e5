"""Per-kernel parity at the edges: the C-ABI entry points that tests/test_kernels.py reaches only through the model-level goldens
(column sums, activation backward, casts, zero fill, the VQA loss / score / row gather, input preparation, attention
probabilities, the rebuild LayerNorm pair, the small-linear heads, the two shadow refreshes, the head dropout), the cross-entropy
paths no kernel test took (scalar rows, the 32768-column boundary of the register-cached path, its pad loop, labels >= V, an
all-ignored batch) and a GEMM sweep over M = 1, N = 1, K < 8 and K % 4 != 0.

Rules of this file:
  * the entry points are called through the C ABI itself (_lib.lib().vb_*), on their own inputs;
  * every reference is plain torch in float64 on the same, already dtype-rounded, inputs;
  * every output lives inside a larger buffer pre-filled with a sentinel (lead and tail elements, extra rows, pad columns of the
    pitch), and everything outside the documented write region must still hold the sentinel afterwards;
  * accumulation targets start non-zero;
  * shapes are the smallest that reach each code path (named next to each case list), not workload sizes.
On a GPU every case records its largest error (profiles/kernel_edges_parity.json is a copy of one such run on MI355X)."""
import math

import pytest
import torch

import golden_util
from visualbert_amd import _lib
from test_kernels import generator_keep

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SENT = 7.0                      # exactly representable in fp32 and bf16
BF16_EPS = 2.0 ** -8            # one bf16 rounding: half an ulp of 2^-7, relative
VB_ERR_UNSUPPORTED = -3


def tol(dt, f32, bf):
    return f32 if dt == torch.float32 else bf


def dname(dt):
    return "f32" if dt == torch.float32 else "bf16"


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def guarded(n, dt, dev, fill=SENT, lead=64, tail=64, sent=SENT):
    """(buffer, view): `view` is n elements inside a sentinel-filled buffer, `lead` elements in (64 elements keep any 16- or
    32-byte alignment of the allocation), itself filled with `fill`."""
    buf = torch.full((lead + n + tail,), sent, dtype=dt, device=dev)
    view = buf[lead:lead + n]
    if fill != sent:
        view.fill_(fill)
    return buf, view


def untouched(buf, n, lead=64, sent=SENT):
    """everything around the n-element view of `guarded` still holds the sentinel"""
    return bool((buf[:lead] == sent).all()) and bool((buf[lead + n:] == sent).all())


def pitched(rows, cols, pad, dt, dev, values=None, padfill=SENT, extra_rows=2):
    """(buffer, view [rows, cols]) with pitch cols + pad, `extra_rows` sentinel rows before and after; pad columns hold `padfill`."""
    ld = cols + pad
    buf = torch.full((rows + 2 * extra_rows, ld), SENT, dtype=dt, device=dev)
    body = buf[extra_rows:extra_rows + rows]
    if pad:
        body[:, cols:] = padfill
    view = body[:, :cols]
    if values is not None:
        view.copy_(values.to(dt).to(dev))
    return buf, view


def outside_untouched(buf, rows, cols, extra_rows=2, padfill=SENT):
    body = buf[extra_rows:extra_rows + rows]
    ok = bool((buf[:extra_rows] == SENT).all()) and bool((buf[extra_rows + rows:] == SENT).all())
    return ok and bool((body[:, cols:] == padfill).all())


def f64(t):
    return t.detach().cpu().double()


def maxerr(a, b):
    return float((f64(a) - f64(b)).abs().max()) if a.numel() else 0.0


def amax1(ref):
    return max(1.0, float(f64(ref).abs().max())) if ref.numel() else 1.0


def record(dev, request, **errs):
    if dev.type == "cuda":
        golden_util.record("kernel_edges", request.node.name, {k: float(v) for k, v in errs.items()},
                           fname="kernel_edges_parity.json")


def within(name, err, bound):
    assert err <= bound, "%s: error %.3e exceeds the bound %.3e (%.1f x)" % (name, err, bound, err / bound)


def sp():
    return _lib.stream_ptr()


def tid(t):
    return "x".join(str(v) for v in t)


# ---- vb_colsum --------------------------------------------------------------------------------------------------------------
# (1,8): one row, one full 8-column lane; (3,5): ragged single lane; 520 / 1030: second 512-column block with a ragged last lane;
# (5000,24): several row blocks (atomics across blockIdx.y); (67,768): the 4-loads-in-flight loop plus its remainder.
# pad 3: a pitch that is no multiple of 8 -> the scalar path; 0 / 8: the 16-byte path where the pitch allows it.
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("pad", [0, 3, 8])
@pytest.mark.parametrize("MN", [(1, 8), (3, 5), (37, 520), (70, 1030), (5000, 24), (67, 768)], ids=tid)
def test_colsum(dev, request, MN, pad, dt):
    M, N = MN
    g = gen(1, M, N, pad)
    xbuf, x = pitched(M, N, pad, dt, dev, torch.randn(M, N, generator=g), padfill=1000.0)
    obuf, out = guarded(N, torch.float32, dev, fill=3.0)
    sc = torch.tensor([0.37], device=dev)
    _lib.check(_lib.lib().vb_colsum(_lib.dtype_code(dt), _lib.ptr(x), x.stride(0), _lib.ptr(out), _lib.ptr(sc), M, N, sp()),
               "vb_colsum")
    ref = 3.0 + float(f64(sc)[0]) * f64(x).sum(0)
    err = maxerr(out, ref)
    record(dev, request, out=err)
    within("out", err, 1e-4 * amax1(ref))
    assert untouched(obuf, N)


# ---- vb_act_bwd -------------------------------------------------------------------------------------------------------------
# 1, 7: scalar tail only; 8: one vector, no tail; 9: vector + tail; 2048: exactly one trip of a block; 2055: a tail behind it;
# 300001: many blocks and a tail
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("act", ["gelu", "tanh"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2048, 2055, 300001])
def test_act_bwd(dev, request, n, act, dt):
    g = gen(2, n, act == "gelu")
    dy = torch.randn(n, generator=g).to(dt).to(dev)
    if act == "gelu":
        aux = (3.0 * torch.randn(n, generator=g)).to(dt).to(dev)
        a = f64(aux)
        d = 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
        code = _lib.VB_ACT_GELU
    else:
        aux = torch.tanh(torch.randn(n, generator=g)).to(dt).to(dev)
        a = f64(aux)
        d = 1.0 - a * a
        code = _lib.VB_ACT_TANH
    ref = f64(dy) * d
    buf, dx = guarded(n, dt, dev)
    _lib.check(_lib.lib().vb_act_bwd(_lib.dtype_code(dt), _lib.ptr(dy), _lib.ptr(aux), _lib.ptr(dx), n, code, sp()), "vb_act_bwd")
    err = maxerr(dx, ref)
    record(dev, request, dx=err)
    within("dx", err, tol(dt, 2e-6, BF16_EPS) * amax1(ref))
    assert untouched(buf, n)


# ---- vb_cast ----------------------------------------------------------------------------------------------------------------
# (n, element offset of both pointers): offsets 1 / 3 break the 16-byte alignment of source and destination -> the element path
# on every group; 4096 / 4099: whole groups, then a ragged last one
@pytest.mark.parametrize("case", [(1, 0), (7, 0), (8, 0), (4096, 0), (1000, 1), (4099, 3)], ids=lambda c: "%d+%d" % c)
@pytest.mark.parametrize("dd", DTYPES, ids=dname)
@pytest.mark.parametrize("sd", DTYPES, ids=dname)
def test_cast(dev, request, sd, dd, case):
    n, off = case
    g = gen(3, n, off)
    vals = torch.randn(n, generator=g)
    # round-to-nearest-even ties of fp32 -> bf16 (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), a value next to a tie, a large one
    special = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.0e38, -0.0, 65280.0])
    k = min(n, special.numel())
    vals[:k] = special[:k]
    src = torch.zeros(n + off + 8, dtype=sd, device=dev)
    src[off:off + n] = vals.to(sd).to(dev)
    lead = 64 + off
    buf = torch.full((lead + n + 64,), SENT, dtype=dd, device=dev)
    dst = buf[lead:lead + n]
    _lib.check(_lib.lib().vb_cast(_lib.dtype_code(sd), _lib.ptr(src[off:]), _lib.dtype_code(dd), _lib.ptr(dst), n, sp()), "vb_cast")
    assert torch.equal(dst, src[off:off + n].to(dd))
    assert untouched(buf, n, lead=lead)
    record(dev, request, exact=0.0)


# ---- vb_zero ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [16, 4096, 16 * 100003])        # one store; one block; several trips of the grid-stride loop, ragged
def test_zero(dev, request, nbytes):
    buf = torch.full((64 + nbytes + 64,), 171, dtype=torch.uint8, device=dev)
    view = buf[64:64 + nbytes]
    _lib.check(_lib.lib().vb_zero(_lib.ptr(view), nbytes, sp()), "vb_zero")
    assert bool((view == 0).all())
    assert untouched(buf, nbytes, sent=171)
    record(dev, request, exact=0.0)


# ---- vb_kldiv_fwd_bwd -------------------------------------------------------------------------------------------------------
def vqa_score_ref(logits, target):
    """compute_score_with_logits of the reference model restated in fp64: softmax, class 0 zeroed (masked_unk_softmax with
    mask_idx 0), renormalised, one-hot of the argmax times the targets; the entry point returns the batch mean."""
    x1 = torch.softmax(logits, 1).clone()
    x1[:, 0] = 0
    y = x1 / x1.sum(1, keepdim=True)
    am = y.max(1)[1]
    one_hot = torch.zeros_like(target)
    one_hot.scatter_(1, am.view(-1, 1), 1.0)
    return float((one_hot * target).sum() / logits.shape[0])


# V = 2: the score can only pick class 1; 255 / 257: one short of / one past a trip of 256 threads; 3129: the VQA answer vocabulary
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("MV", [(3, 2), (5, 255), (4, 257), (3, 3129)], ids=tid)
def test_kldiv_loss_score_gradient(dev, request, MV, pad):
    M, V = MV
    L = _lib.lib()
    g = gen(4, M, V, pad)
    xv = 2.0 * torch.randn(M, V, generator=g)
    tv = torch.zeros(M, V)
    picks = [0.3, 0.6, 1.0]
    for r in range(1, M):                                       # row 0: an all-zero target
        for j in range(min(3, V)):
            tv[r, int(torch.randint(0, V, (1,), generator=g))] = picks[j]
    for r in range(2, M):                                       # the scored class (best of 1..V-1) carries a target on these rows
        tv[r, 1 + int(xv[r, 1:].argmax())] = 0.9
    # row 1: the largest raw logit is class 0, which the score must ignore; class 0 carries the largest target, the class the
    # score must pick a different one
    xv[1, 0] = float(xv[1].max()) + 5.0
    tv[1, 0] = 1.0
    tv[1, 1 + int(xv[1, 1:].argmax())] = 0.3
    xbuf, x = pitched(M, V, pad, torch.float32, dev, xv, padfill=50.0)
    tbuf, t = pitched(M, V, pad, torch.float32, dev, tv, padfill=0.5)
    xr = f64(x).requires_grad_(True)
    ref = torch.nn.functional.kl_div(torch.log_softmax(xr, 1), f64(t), reduction="batchmean")
    ref.backward()
    ref = ref.detach()
    ref_score = vqa_score_ref(f64(x), f64(t))
    assert ref_score > 0.0 and abs(ref_score - float((f64(t) * torch.nn.functional.one_hot(f64(x).argmax(1), V)).sum()) / M) > 1e-3

    def run(with_score, with_grad):
        sbuf, s = guarded(2, torch.float32, dev, lead=1, tail=1)           # {loss, score}
        dbuf, d = pitched(M, V, pad, torch.float32, dev)
        _lib.check(L.vb_kldiv_fwd_bwd(_lib.ptr(x), x.stride(0), _lib.ptr(t), t.stride(0), _lib.ptr(s[0:]), _lib.ptr(s[1:]) if with_score else None,
                                      _lib.ptr(d) if with_grad else None, d.stride(0), M, V, sp()), "vb_kldiv_fwd_bwd")
        assert untouched(sbuf, 2, lead=1)
        assert outside_untouched(dbuf, M, V)
        return s, d

    s, d = run(True, True)
    e_loss = abs(float(s[0]) - float(ref)) / max(1.0, abs(float(ref)))
    e_grad = maxerr(d, xr.grad)
    e_score = abs(float(s[1]) - ref_score)
    record(dev, request, loss_rel=e_loss, dlogits=e_grad, score=e_score)
    within("loss", e_loss, 1e-5)
    within("dlogits", e_grad, 1e-6)
    within("score", e_score, 1e-6)
    s, d = run(False, True)                                     # score = NULL: its slot stays as it was
    assert float(s[1]) == SENT
    within("loss, no score", abs(float(s[0]) - float(ref)), 1e-5 * max(1.0, abs(float(ref))))
    within("dlogits, no score", maxerr(d, xr.grad), 1e-6)
    s, d = run(True, False)                                     # dlogits = NULL: nothing of the gradient buffer is written
    assert bool((d == SENT).all())
    within("loss, no gradient", abs(float(s[0]) - float(ref)), 1e-5 * max(1.0, abs(float(ref))))
    within("score, no gradient", abs(float(s[1]) - ref_score), 1e-6)


# ---- vb_gather_rows / vb_scatter_rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
def test_gather_and_scatter_rows(dev, request, dt):
    """H = 264: a second, ragged trip of the 256 threads; mask length 2 -> row 0, length T -> the last text row"""
    L = _lib.lib()
    B, T, R, H = 5, 9, 4, 264
    S = T + R
    lens = [9, 2, 5, 3, 7]
    g = gen(5)
    x = torch.randn(B, S, H, generator=g).to(dt).to(dev)
    mask = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    mask = mask.to(dev)
    obuf, out = guarded(B * H, dt, dev)
    ibuf, idx = guarded(B, torch.int64, dev, sent=-77, fill=-77)
    _lib.check(L.vb_gather_rows(_lib.dtype_code(dt), _lib.ptr(x), _lib.ptr(mask), _lib.ptr(out), _lib.ptr(idx), B, S, T, H, sp()),
               "vb_gather_rows")
    want_idx = torch.tensor([n - 2 for n in lens])
    assert torch.equal(idx.cpu(), want_idx)
    assert torch.equal(out.view(B, H).cpu(), x.cpu()[torch.arange(B), want_idx])
    assert untouched(obuf, B * H) and untouched(ibuf, B, sent=-77)
    dout = torch.randn(B, H, generator=g).to(dt).to(dev)
    dbuf, dx = guarded(B * S * H, dt, dev)
    _lib.check(L.vb_scatter_rows(_lib.dtype_code(dt), _lib.ptr(dout), _lib.ptr(idx), _lib.ptr(dx), B, S, H, sp()), "vb_scatter_rows")
    want = torch.full((B, S, H), SENT, dtype=dt)                # the entry writes the B selected rows and nothing else
    want[torch.arange(B), want_idx] = dout.cpu()
    assert torch.equal(dx.view(B, S, H).cpu(), want)
    assert untouched(dbuf, B * S * H)
    record(dev, request, exact=0.0)


# ---- vb_prepare_inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_labels", [True, False], ids=["labels", "nolabels"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["imagemask", "imagedim"])
def test_prepare_inputs(dev, request, with_mask, with_labels):
    """image_dim = 0 (no region), 3 (some), 9 > R (all) on the three samples; image_mask, when given, wins over image_dim"""
    L = _lib.lib()
    B, T, R = 3, 7, 5
    S = T + R
    g = gen(6, with_mask, with_labels)
    input_mask = torch.randint(0, 2, (B, T), generator=g)
    image_dim = torch.tensor([0, 3, 9])
    image_mask = torch.randint(0, 2, (B, R), generator=g) if with_mask else None
    labels = torch.randint(-1, 50, (B, T), generator=g) if with_labels else None
    vis = image_mask if with_mask else (torch.arange(R).view(1, R) < image_dim.view(B, 1)).long()
    want_mask = torch.cat((input_mask, vis), 1)
    want_add = ((1.0 - want_mask.float()) * -10000.0)
    want_lab = torch.cat((labels if with_labels else torch.full((B, T), -1), torch.full((B, R), -1)), 1)
    d = lambda t: None if t is None else t.to(dev)
    im, idim, imask, lab = d(input_mask), d(image_dim), d(image_mask), d(labels)
    abuf, am = guarded(B * S, torch.int64, dev, sent=-77, fill=-77)
    fbuf, ma = guarded(B * S, torch.float32, dev)
    lbuf, le = guarded(B * S, torch.int64, dev, sent=-77, fill=-77)
    _lib.check(L.vb_prepare_inputs(_lib.ptr(im), _lib.ptr(idim), _lib.ptr(imask), _lib.ptr(lab), _lib.ptr(am), _lib.ptr(ma), _lib.ptr(le),
                                   B, T, R, sp()), "vb_prepare_inputs")
    assert torch.equal(am.view(B, S).cpu(), want_mask)
    assert torch.equal(ma.view(B, S).cpu(), want_add)
    assert torch.equal(le.view(B, S).cpu(), want_lab)
    assert untouched(abuf, B * S, sent=-77) and untouched(fbuf, B * S) and untouched(lbuf, B * S, sent=-77)
    le.fill_(-77)                                               # labels_ext = NULL: the other two outputs as before, nothing else
    am.fill_(-77)
    _lib.check(L.vb_prepare_inputs(_lib.ptr(im), _lib.ptr(idim), _lib.ptr(imask), _lib.ptr(lab), _lib.ptr(am), _lib.ptr(ma), None,
                                   B, T, R, sp()), "vb_prepare_inputs")
    assert torch.equal(am.view(B, S).cpu(), want_mask) and bool((lbuf == -77).all())
    record(dev, request, exact=0.0)


# ---- vb_attn_probs ----------------------------------------------------------------------------------------------------------
# S = 5: a fraction of one trip; 64: one wave; 257 / 300: a second trip of the score, exponential and normalising loops
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("cfg", [(2, 5, 1), (2, 64, 3), (1, 257, 2), (1, 300, 1)], ids=tid)
def test_attn_probs(dev, request, cfg, dt):
    B, S, nh = cfg
    d = 64
    H = nh * d
    g = gen(7, B, S, nh)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(dt).to(dev)
    keep = torch.rand(B, S, generator=g) < 0.7
    keep[:, 0] = True
    mask_add = ((1.0 - keep.float()) * -10000.0).to(dev)
    n = B * nh * S * S
    buf, probs = guarded(n, torch.float32, dev)
    _lib.check(_lib.lib().vb_attn_probs(_lib.dtype_code(dt), _lib.ptr(qkv), _lib.ptr(mask_add), _lib.ptr(probs), B, S, nh, d, sp()),
               "vb_attn_probs")
    q, k, _ = [t.view(B, S, nh, d).permute(0, 2, 1, 3) for t in f64(qkv).view(B, S, 3 * H).split(H, dim=-1)]
    ref = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + f64(mask_add).view(B, 1, 1, S), -1)
    err = maxerr(probs.view(B, nh, S, S), ref)
    record(dev, request, probs=err)
    within("probs", err, 5e-6)
    assert untouched(buf, n)


# ---- vb_ln_fwd_rb / vb_ln_bwd_rb --------------------------------------------------------------------------------------------
def ln_params(kind, H, g):
    """(gamma, beta, verdict the forward must reach): rebuild allowed iff 1e-30 < |gamma| and |beta| <= 2 |gamma| on every channel"""
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    if kind == "init":
        return gamma, beta, 1
    if kind == "negated":                                   # the sign of gamma must not matter; one small positive channel
        gamma = -gamma
        gamma[3], beta[3] = 0.05, 0.08
        return gamma, beta, 1
    if kind == "beta2.5":
        beta[H - 5] = -2.5 * gamma[H - 5].abs()
        return gamma, beta, 0
    if kind == "zero":
        gamma[H // 2 + 1], beta[H // 2 + 1] = 0.0, 0.0
        return gamma, beta, 0
    assert kind == "trained"
    gamma = 0.3 * gamma
    beta = torch.randn(H, generator=g)
    lim = 1.9 * gamma.abs()
    beta = torch.max(torch.min(beta, lim), -lim)
    return gamma, beta, 1


def ln_ref(z, gamma, beta):
    u = z.mean(-1, keepdim=True)
    s = (z - u).pow(2).mean(-1, keepdim=True)
    return gamma * ((z - u) / torch.sqrt(s + 1e-12)) + beta


# H = 64: a quarter of the lanes; 128 / 256: one chunk per lane; 640 / 768: the twelve-columns-per-lane backward (640: a partly filled
# 4-column chunk); M = 300: several workgroups and trips
@pytest.mark.parametrize("kind", ["init", "negated", "beta2.5", "zero", "trained"])
@pytest.mark.parametrize("two_stage", [True, False], ids=["ws", "atomics"])
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("MH", [(5, 64), (37, 128), (300, 256), (13, 640), (21, 768)], ids=tid)
def test_layernorm_rebuild_pair(dev, request, MH, dt, two_stage, kind):
    M, H = MH
    L = _lib.lib()
    code = _lib.dtype_code(dt)
    g = gen(8, M, H)
    x = torch.randn(M, H, generator=g).to(dt).to(dev)
    r = torch.randn(M, H, generator=g).to(dt).to(dev)
    dy = torch.randn(M, H, generator=g).to(dt).to(dev)
    gamma, beta, verdict = ln_params(kind, H, g)
    gamma, beta = gamma.to(dev), beta.to(dev)
    n = M * H
    zbuf, z = guarded(n, dt, dev)
    ybuf, y = guarded(n, dt, dev)
    mbuf, mean = guarded(M, torch.float32, dev)
    rbuf, rstd = guarded(M, torch.float32, dev)
    vbuf, rb = guarded(1, torch.int32, dev, sent=-77, fill=-77)
    _lib.check(L.vb_ln_fwd_rb(code, _lib.ptr(x), _lib.ptr(r), _lib.ptr(z), _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma),
                              _lib.ptr(beta), M, H, 1e-12, 0.0, 11, 5, _lib.ptr(rb), sp()), "vb_ln_fwd_rb")
    assert int(rb[0]) == verdict
    assert untouched(zbuf, n) and untouched(ybuf, n) and untouched(mbuf, M) and untouched(rbuf, M) and untouched(vbuf, 1, sent=-77)
    z_exact = f64(x) + f64(r)
    errs = {}
    if verdict:
        assert bool((z == SENT).all())                          # three tensors per launch: the pre-LN sum is not written
        zs = z_exact
    else:
        errs["z"] = maxerr(z.view(M, H), z_exact)
        within("z", errs["z"], tol(dt, 1e-6, 0.04))
        zs = f64(z).view(M, H)                                  # the backward consumes the stored (T-rounded) sum: so does the reference
    errs["y"] = maxerr(y.view(M, H), ln_ref(z_exact, f64(gamma), f64(beta)))
    within("y", errs["y"], tol(dt, 2e-5, 0.04))
    zs = zs.clone().requires_grad_(True)
    gp, bp = f64(gamma).requires_grad_(True), f64(beta).requires_grad_(True)
    ln_ref(zs, gp, bp).backward(f64(dy))
    dzbuf, dz = guarded(n, dt, dev)
    dxbuf, dx = guarded(n, dt, dev)
    acc = [guarded(H, torch.float32, dev, fill=1.0) for _ in range(3)]
    ws = torch.empty(L.vb_ln_bwd_ws_bytes(M, H) // 4, device=dev) if two_stage else None
    _lib.check(L.vb_ln_bwd_rb(code, _lib.ptr(dy), _lib.ptr(z), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(dz), _lib.ptr(dx),
                              _lib.ptr(acc[0][1]), _lib.ptr(acc[1][1]), _lib.ptr(acc[2][1]), M, H, 0.0, 11, 5, _lib.ptr(ws),
                              _lib.ptr(y), _lib.ptr(beta), _lib.ptr(rb), sp()), "vb_ln_bwd_rb")
    assert untouched(dzbuf, n) and untouched(dxbuf, n) and all(untouched(b, H) for b, _ in acc)
    refs = {"dz": zs.grad, "dgamma": 1.0 + gp.grad, "dbeta": 1.0 + bp.grad, "dbias": 1.0 + zs.grad.sum(0)}
    got = {"dz": dz.view(M, H), "dgamma": acc[0][1], "dbeta": acc[1][1], "dbias": acc[2][1]}
    bound = {"dz": tol(dt, 5e-5, 0.05), "dgamma": tol(dt, 2e-4, 0.02), "dbeta": 2e-4, "dbias": tol(dt, 2e-4, 0.01)}
    for k in refs:
        errs[k] = maxerr(got[k], refs[k]) / amax1(refs[k] - (0.0 if k == "dz" else 1.0))
    record(dev, request, **errs)
    for k in refs:
        within(k, errs[k], bound[k])
    assert torch.equal(dx, dz)


# ---- vb_small_linear_fwd / _bwd ---------------------------------------------------------------------------------------------
# M > 32: several row slices of the dW / db reductions (70: a ragged last slice, 200: seven); (33,3,100), (200,2,40): M K > N K,
# (1,1,8), (5,4,1030): the reverse or equal -- the grid is sized by the larger; pitch K + 8: pad columns in x and dx
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("MNK", [(1, 1, 8), (33, 3, 100), (70, 2, 768), (200, 2, 40), (5, 4, 1030)], ids=tid)
def test_small_linear_fwd_bwd(dev, request, MNK, pad, dt):
    M, N, K = MNK
    L = _lib.lib()
    code = _lib.dtype_code(dt)
    g = gen(9, M, N, K, pad)
    xbuf, x = pitched(M, K, pad, dt, dev, torch.randn(M, K, generator=g), padfill=1000.0)
    W = torch.randn(N, K, generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    dy = torch.randn(M, N, generator=g).to(dev)
    ybuf, y = guarded(M * N, torch.float32, dev)
    _lib.check(L.vb_small_linear_fwd(code, _lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(bias), _lib.ptr(y), M, N, K, sp()),
               "vb_small_linear_fwd")
    ref_y = f64(x) @ f64(W).t() + f64(bias)
    errs = {"y": maxerr(y.view(M, N), ref_y) / amax1(ref_y)}
    assert untouched(ybuf, M * N)
    sc = torch.tensor([0.25], device=dev)
    dxbuf, dx = pitched(M, K, pad, dt, dev)
    wbuf, dW = guarded(N * K, torch.float32, dev, fill=2.0)
    bbuf, db = guarded(N, torch.float32, dev, fill=2.0)
    _lib.check(L.vb_small_linear_bwd(code, _lib.ptr(dy), _lib.ptr(x), x.stride(0), _lib.ptr(W), _lib.ptr(dx), dx.stride(0), _lib.ptr(dW),
                                     _lib.ptr(db), _lib.ptr(sc), M, N, K, sp()), "vb_small_linear_bwd")
    ref_dx = 0.25 * (f64(dy) @ f64(W))
    ref_dW = 2.0 + 0.25 * (f64(dy).t() @ f64(x))
    ref_db = 2.0 + 0.25 * f64(dy).sum(0)
    errs["dx"] = maxerr(dx, ref_dx) / amax1(ref_dx)
    errs["dW"] = maxerr(dW.view(N, K), ref_dW) / amax1(ref_dW)
    errs["db"] = maxerr(db, ref_db) / amax1(ref_db)
    record(dev, request, **errs)
    for k in ("y", "dW", "db"):
        within(k, errs[k], 1e-4)
    within("dx", errs["dx"], tol(dt, 1e-5, BF16_EPS))
    assert outside_untouched(dxbuf, M, K) and untouched(wbuf, N * K) and untouched(bbuf, N)
    # dx = NULL, dW = NULL: only the bias gradient moves
    db.fill_(2.0)
    _lib.check(L.vb_small_linear_bwd(code, _lib.ptr(dy), _lib.ptr(x), x.stride(0), _lib.ptr(W), None, 0, None,
                                     _lib.ptr(db), _lib.ptr(sc), M, N, K, sp()), "vb_small_linear_bwd")
    within("db alone", maxerr(db, ref_db), 1e-4 * amax1(ref_db))


# ---- vb_refresh_transposed_shadow / vb_refresh_bf16_shadow ------------------------------------------------------------------
def test_refresh_transposed_shadow(dev, request):
    """W^T copies through 64 x 64 tiles, one call over six tensors: (130,72) interior and ragged tiles in both directions, (64,64) one
    interior tile on the 16-byte path, (58,200) no full row tile, (1,8) a single row, (70,13) with a source offset that is no multiple
    of 8, and a second (64,64) at such an offset: an interior tile that must take the element-wise path.  Exact; the pad columns
    R .. ld-1 of every destination row and the gaps between the tensors keep the sentinel."""
    g = gen(10)
    shapes = [(130, 72), (64, 64), (58, 200), (1, 8), (70, 13), (64, 64)]
    misaligned = {4: 3, 5: 5}
    tens, tiles, soff, doff = [], [], 0, 0
    for i, (R, C) in enumerate(shapes):
        soff = (soff + 7) // 8 * 8 + misaligned.get(i, 0)
        ld = (R + 7) // 8 * 8 + 8
        tens.append([soff, R, C, doff, ld])
        for tr in range((R + 63) // 64):
            for tc in range((C + 63) // 64):
                tiles.append([i, tr, tc])
        soff += R * C
        doff += C * ld + 8                                      # a gap of 8 elements behind every destination
    src = torch.randn(soff + 8, generator=g).to(torch.bfloat16)
    want = torch.full((doff,), SENT, dtype=torch.bfloat16)
    for so, R, C, do, ld in tens:
        want[do:do + C * ld].view(C, ld)[:, :R] = src[so:so + R * C].view(R, C).t()
    srcd = src.to(dev)
    dbuf, dst = guarded(doff, torch.bfloat16, dev)
    tt = torch.tensor(tens, dtype=torch.int64).to(dev)
    tl = torch.tensor(tiles, dtype=torch.int64).to(dev)
    _lib.check(_lib.lib().vb_refresh_transposed_shadow(_lib.ptr(srcd), _lib.ptr(dst), _lib.ptr(tt), _lib.ptr(tl), len(tiles), sp()),
               "vb_refresh_transposed_shadow")
    assert torch.equal(dst.cpu(), want)
    assert untouched(dbuf, doff)
    record(dev, request, exact=0.0)


def test_refresh_bf16_shadow(dev, request):
    """three tensors: a 1-D one without a shadow (offset -1: nothing of it may be written), one of 40,000 elements over three chunks
    (ragged last chunk), one small matrix; round-to-nearest-even, ties included"""
    g = gen(11)
    CHUNK = 16384
    numel = [37, 40000, 100]
    t_off = [0, 40, 40048]
    sh_off = [-1, 16, 16 + 40000 + 8]
    n_shadow = sh_off[2] + 100 + 8
    params = torch.randn(t_off[2] + 100, generator=g)
    params[40:44] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23])
    tens, chunks = [], []
    for i in range(3):
        tens.append([t_off[i], numel[i], sh_off[i], 1])
        cnt = (numel[i] + CHUNK - 1) // CHUNK
        for s in range(0, numel[i], CHUNK):
            chunks.append([i, t_off[i] + s, min(CHUNK, numel[i] - s), cnt])
    want = torch.full((n_shadow,), SENT, dtype=torch.bfloat16)
    for i in (1, 2):
        want[sh_off[i]:sh_off[i] + numel[i]] = params[t_off[i]:t_off[i] + numel[i]].to(torch.bfloat16)
    pd = params.to(dev)
    sbuf, shadow = guarded(n_shadow, torch.bfloat16, dev)
    tt = torch.tensor(tens, dtype=torch.int64).to(dev)
    ct = torch.tensor(chunks, dtype=torch.int64).to(dev)
    _lib.check(_lib.lib().vb_refresh_bf16_shadow(_lib.ptr(pd), _lib.ptr(shadow), _lib.ptr(ct), len(chunks), _lib.ptr(tt), sp()),
               "vb_refresh_bf16_shadow")
    assert torch.equal(shadow.cpu(), want)
    assert untouched(sbuf, n_shadow)
    record(dev, request, exact=0.0)


# ---- vb_dropout -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("n", [1, 7, 4099])                 # a fraction of one generator group; whole groups and a ragged last one
def test_dropout_direct(dev, request, n, dt):
    """vb_dropout on its own inputs: the keep mask is the documented generator's, kept values are x / (1 - p) rounded once (one fp32
    multiply by the fp32 reciprocal, then the conversion to T), in place works, the tail is untouched"""
    import numpy as np
    p, seed, sid = 0.25, (3 << 32) | 77, 9
    x = torch.linspace(1.0, 2.0, n).to(dt).to(dev)
    buf, y = guarded(n, dt, dev)
    code = _lib.dtype_code(dt)
    _lib.check(_lib.lib().vb_dropout(code, _lib.ptr(x), _lib.ptr(y), n, p, seed, sid, sp()), "vb_dropout")
    keep = torch.from_numpy(generator_keep(np.arange((n + 7) // 8), p, seed, sid).reshape(-1)[:n].copy())
    inv_keep = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    want = torch.where(keep, (x.cpu().float() * torch.tensor(inv_keep)).to(dt), torch.zeros(n, dtype=dt))
    assert torch.equal(y.cpu(), want)
    assert untouched(buf, n)
    _lib.check(_lib.lib().vb_dropout(code, _lib.ptr(x), _lib.ptr(x), n, p, seed, sid, sp()), "vb_dropout")
    assert torch.equal(x.cpu(), want)
    record(dev, request, exact=0.0)


# ---- cross-entropy edges ----------------------------------------------------------------------------------------------------
# (M, V, ld_logits, ld_dlogits).  Pitch 2 (image-text match, NLVR2) and 4 (multichoice): the scalar path; V = 3 in a pitch of 8: the
# vector path on a row shorter than one vector; 1001 / 1003: odd pitches, the scalar path at a vocabulary-sized row; 1024 / 1088:
# dlogits with more pad columns than the logits; 32761, 32768, 32769: around the 32768 columns the register-cached path holds
# (32768 with a pitch of 32832: its "pad beyond the cached span" loop; 32769: the first row of the rolled two-pass path); 40000:
# the rolled path with pad columns
CE_CASES = [(5, 2, 2, 2), (6, 4, 4, 4), (7, 3, 8, 8), (9, 1001, 1001, 1003), (9, 1000, 1024, 1088), (3, 32761, 32768, 32768),
            (4, 32768, 32768, 32832), (3, 32769, 32776, 32776), (3, 40000, 40000, 40064)]


def ce_ref(x, lab, V):
    """CrossEntropyLoss(ignore_index = -1) in fp64, mean over the counted rows; a label outside [0, V) counts as ignored"""
    counted = (lab >= 0) & (lab < V)
    n = int(counted.sum())
    lsm = torch.log_softmax(x, 1)
    grad = torch.zeros_like(x)
    if n == 0:
        return float("nan"), grad
    rows = torch.nonzero(counted).reshape(-1)
    loss = -lsm[rows, lab[rows]].sum() / n
    grad[rows] = torch.exp(lsm[rows])
    grad[rows, lab[rows]] -= 1.0
    return float(loss), grad / n


@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("scale", [3, 3000])
@pytest.mark.parametrize("case", CE_CASES, ids=lambda c: "%dx%d_ld%d_%d" % c)
def test_cross_entropy_edges(dev, request, case, scale, dt):
    M, V, ld, ldd = case
    L = _lib.lib()
    code = _lib.dtype_code(dt)
    g = gen(12, M, V, scale)
    logits = torch.full((M, ld), 1e30)                          # pad columns must be ignored
    logits[:, :V] = scale * torch.randn(M, V, generator=g)
    logits = logits.to(dev)
    x64 = f64(logits)[:, :V]
    base = [0, V - 1, -1, V + 5] + [int(v) for v in torch.randint(0, V, (max(0, M - 4),), generator=g)]
    label_sets = [base[:M]] if M >= 4 else [base[:M], [V + 5, V - 1, 0][:M]]
    label_sets.append([-1] * M)                                 # an all-ignored batch: NaN loss, all-zero gradient
    errs = {"loss_rel": 0.0, "dlogits": 0.0}
    for labels in label_sets:
        lab = torch.tensor(labels, dtype=torch.int64)
        ref_loss, ref_grad = ce_ref(x64, lab, V)
        labd = lab.to(dev)
        abuf, acc = guarded(66, torch.float32, dev)
        lbuf, loss = guarded(1, torch.float32, dev)
        dbuf = torch.full((M + 4, ldd), SENT, dtype=dt, device=dev)         # two sentinel rows before and after
        dl = dbuf[2:2 + M]
        _lib.check(L.vb_ce_fwd_bwd(code, _lib.ptr(logits), ld, _lib.ptr(labd), -1, _lib.ptr(acc), _lib.ptr(loss), _lib.ptr(dl), ldd, M, V, sp()),
                   "vb_ce_fwd_bwd")
        assert untouched(abuf, 66) and untouched(lbuf, 1)
        assert bool((dbuf[:2] == SENT).all()) and bool((dbuf[2 + M:] == SENT).all())
        assert bool((dl[:, V:].float() == 0).all())             # pad columns of the gradient are written as zeros
        lbuf2, loss2 = guarded(1, torch.float32, dev)
        _lib.check(L.vb_ce_fwd_bwd(code, _lib.ptr(logits), ld, _lib.ptr(labd), -1, _lib.ptr(acc), _lib.ptr(loss2), None, 0, M, V, sp()),
                   "vb_ce_fwd_bwd")
        if math.isnan(ref_loss):
            assert math.isnan(float(loss[0])) and math.isnan(float(loss2[0]))
            assert bool((dl.float() == 0).all())
            continue
        e_loss = max(abs(float(loss[0]) - ref_loss), abs(float(loss2[0]) - ref_loss)) / max(1.0, abs(ref_loss))
        e_grad = maxerr(dl[:, :V], ref_grad)
        errs["loss_rel"], errs["dlogits"] = max(errs["loss_rel"], e_loss), max(errs["dlogits"], e_grad)
        within("loss %s" % labels[:4], e_loss, 2e-5)
        within("dlogits %s" % labels[:4], e_grad, tol(dt, 2e-6, 2e-3))
    record(dev, request, **errs)


# ---- GEMM edge sweep --------------------------------------------------------------------------------------------------------
# M = 1 / N = 1 / K = 1; K = 4, 12, 20, 36, 68, 100: K % 8 != 0 (the masked last 16-byte chunk of a bf16 row) and K < 8; 63 / 65 / 129 /
# 257: one short of / one past a tile edge; (256,256,64): whole tiles, the pipelined kernels; 776: a long ragged reduction
GEMM_SHAPES = [(1, 1, 1), (1, 8, 8), (7, 1, 12), (63, 65, 36), (65, 63, 100), (129, 30, 4), (2, 257, 776), (257, 129, 72),
               (256, 256, 64), (300, 2, 68), (5, 520, 20)]
GEMM_LAYOUTS = [(0, 0), (0, 1), (1, 1)]                     # (A, B): VB_KCONTIG / VB_KSTRIDED


def gemm_operand(rows, K, layout, dt, dev, g):
    """(tensor handed to the ABI, fp64 [rows, K] matrix it stands for): K-contiguous [rows, round_up(K, 8)] or K-strided
    [K, round_up(rows, 8)]; the columns beyond K / rows -- which the ABI only asks to be readable -- hold 77"""
    vals = torch.randn(rows, K, generator=g).to(dt)
    if layout == _lib.VB_KCONTIG:
        t = torch.full((rows, (K + 7) // 8 * 8), 77.0, dtype=dt)
        t[:, :K] = vals
    else:
        t = torch.full((K, (rows + 7) // 8 * 8), 77.0, dtype=dt)
        t[:, :rows] = vals.t()
    return t.to(dev), vals.double()


def gemm_call(dt, out_dt, al, bl, A, B, C, M, N, K, bias, colsum):
    return _lib.lib().vb_gemm(_lib.dtype_code(dt), _lib.dtype_code(out_dt), al, bl, _lib.ptr(A), A.stride(0), _lib.ptr(B), B.stride(0),
                              _lib.ptr(C), C.stride(0), M, N, K, 0.5, None, _lib.ptr(bias), None, 0, _lib.VB_ACT_NONE, None, None, 0, 0,
                              _lib.ptr(colsum), sp())


def gemm_c_buffer(M, N, out_dt, dev):
    """C [M, N] inside a sentinel buffer: two rows before and after, a pitch with pad columns -- 16-byte aligned rows for odd M, an odd
    pitch for even M"""
    ldc = ((N + 7) // 8 * 8 + 8) if (M & 1) else N + 3
    buf = torch.full((M + 4, ldc), SENT, dtype=out_dt, device=dev)
    return buf, buf[2:2 + M, :N]


@pytest.mark.parametrize("out_f32", [True, False], ids=["out_f32", "out_same"])
@pytest.mark.parametrize("dt", DTYPES, ids=dname)
@pytest.mark.parametrize("layouts", GEMM_LAYOUTS, ids=lambda l: "a%db%d" % l)
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_gemm_edge_sweep(dev, request, shape, layouts, dt, out_f32):
    M, N, K = shape
    al, bl = layouts
    out_dt = torch.float32 if out_f32 else dt
    g = gen(13, M, N, K)
    A, a64 = gemm_operand(M, K, al, dt, dev, g)
    B, b64 = gemm_operand(N, K, bl, dt, dev, g)
    bias = torch.randn(N, generator=g).to(dev)
    cbuf, C = gemm_c_buffer(M, N, out_dt, dev)
    sbuf, cs = guarded(N, torch.float32, dev, fill=1.0)
    _lib.check(gemm_call(dt, out_dt, al, bl, A, B, C, M, N, K, bias, cs), "vb_gemm")
    ref = 0.5 * (a64 @ b64.t()) + f64(bias)
    factor = max(1.0, math.sqrt(K) / 4.0)
    err = maxerr(C, ref)
    ref_cs = 1.0 + f64(C).sum(0)                                # the column sums are those of the values WRITTEN to C
    err_cs = maxerr(cs, ref_cs) / amax1(ref_cs)
    record(dev, request, c=err, colsum=err_cs)
    within("C", err, (1e-4 if out_dt == torch.float32 else BF16_EPS * amax1(ref)) * factor)
    within("colsum", err_cs, 1e-3 if out_dt == torch.float32 else 0.05)
    assert bool((cbuf[:2] == SENT).all()) and bool((cbuf[2 + M:] == SENT).all()) and bool((cbuf[2:2 + M, N:] == SENT).all())
    assert untouched(sbuf, N)


@pytest.mark.parametrize("dt", DTYPES, ids=dname)
def test_gemm_a_kstrided_b_kcontig_is_unsupported(dev, request, dt):
    """the fourth layout pair has no kernel: VB_ERR_UNSUPPORTED, nothing written (include/visualbert_hip.h says so)"""
    M, N, K = 65, 63, 100
    g = gen(14)
    A, _ = gemm_operand(M, K, _lib.VB_KSTRIDED, dt, dev, g)
    B, _ = gemm_operand(N, K, _lib.VB_KCONTIG, dt, dev, g)
    bias = torch.randn(N, generator=g).to(dev)
    for out_dt in (torch.float32, dt):
        cbuf, C = gemm_c_buffer(M, N, out_dt, dev)
        sbuf, cs = guarded(N, torch.float32, dev, fill=1.0)
        assert gemm_call(dt, out_dt, _lib.VB_KSTRIDED, _lib.VB_KCONTIG, A, B, C, M, N, K, bias, cs) == VB_ERR_UNSUPPORTED
        assert bool((cbuf == SENT).all()) and bool((cs == 1.0).all()) and untouched(sbuf, N)
    record(dev, request, exact=0.0)
