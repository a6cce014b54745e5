"""The one-pass bf16 attention backward (attention.hip: attn_bwd_resident_kernel, 64 < S <= 192, two workgroups per CU) against
the plain fp32 restatement of modeling.py:236-256, at the bf16 bounds of test_kernels.py, over every key-fragment count it serves
and both ragged edges of each; plus bit-repeatability of dqkv and of the per-sample bias-gradient sums."""
import pytest
import torch

from visualbert_amd import _lib
from test_kernels import ATTN_BF16_CTX, ATTN_BF16_DQKV, attn_ref, decode_keepbits

# NKF = ceil(S / 16) = 5 ... 12, each at its first and its last length
LENGTHS = [65, 80, 81, 96, 97, 112, 113, 128, 129, 144, 145, 160, 161, 164, 176, 177, 192]
NH = 12


def _case(dev, B, S, p, seed):
    H = NH * 64
    g = torch.Generator().manual_seed(seed)
    qkv = (0.7 * torch.randn(B, S, 3 * H, generator=g)).to(torch.bfloat16).to(dev)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    mask = (torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)).float()
    mask[:, S // 3] = 0
    mask_add = ((1 - mask) * -10000.0).to(dev)
    dctx = torch.randn(B, S, H, generator=g).to(torch.bfloat16).to(dev)
    L = _lib.lib()
    ctx = torch.empty(B, S, H, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, NH, S, device=dev)
    bits = torch.zeros(B * NH * L.vb_attn_keepbits_words(S), dtype=torch.int64, device=dev)
    _lib.check(L.vb_attn_fwd(_lib.VB_BF16, _lib.ptr(qkv), _lib.ptr(mask_add), _lib.ptr(ctx), _lib.ptr(lse), _lib.ptr(bits),
                             B, S, NH, 64, p, 91, 5, _lib.stream_ptr()), "vb_attn_fwd")
    return dict(B=B, S=S, p=p, qkv=qkv, mask_add=mask_add, dctx=dctx, ctx=ctx, lse=lse, bits=bits)


def _bwd(c, with_bias, stream=None):
    """one-pass backward (the forward output is given): dqkv, with_bias the q|k|v bias gradient added onto 2.0, and the workspace
    (with_bias: the kernel's per-sample column sums [B][3H])"""
    L = _lib.lib()
    B, S, dev = c["B"], c["S"], c["qkv"].device
    dqkv = torch.full((B, S, 3 * NH * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    ws = torch.empty(L.vb_attn_bwd_ws_floats(B, S, NH), device=dev)
    dbias = torch.full((3 * NH * 64,), 2.0, device=dev)
    rc = L.vb_attn_bwd(_lib.VB_BF16, _lib.ptr(c["qkv"]), _lib.ptr(c["mask_add"]), _lib.ptr(c["dctx"]), _lib.ptr(c["lse"]),
                       _lib.ptr(c["bits"]), _lib.ptr(ws), _lib.ptr(dqkv), _lib.ptr(c["ctx"]),
                       _lib.ptr(dbias) if with_bias else None, B, S, NH, 64, c["p"], 91, 5,
                       _lib.stream_ptr() if stream is None else stream)
    _lib.check(rc, "vb_attn_bwd")
    return dqkv, dbias, ws


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", LENGTHS)
def test_resident_bwd_matches_fp32_reference(dev, S, p):
    B = 16 if dev.type == "cuda" else 2          # (the kernel-logic simulator: two samples keep 24 workgroups)
    c = _case(dev, B, S, p, 1000 + S)
    keep = decode_keepbits(c["bits"], B, NH, S).to(dev).float() if p > 0 else None
    qr = c["qkv"].float().detach().requires_grad_(True)
    ctx_r, _ = attn_ref(qr, c["mask_add"], NH, keep, p)
    assert (c["ctx"].float() - ctx_r).abs().max().item() <= ATTN_BF16_CTX
    ctx_r.backward(c["dctx"].float())
    gmax = qr.grad.abs().max().item()
    bias_ref = qr.grad.sum(dim=(0, 1))
    for with_bias in (False, True):
        dqkv, dbias, _ = _bwd(c, with_bias)
        err = (dqkv.float() - qr.grad).abs().max().item()
        assert err <= ATTN_BF16_DQKV * max(1.0, gmax), (err, gmax, with_bias)
        if with_bias:
            berr = (dbias - 2.0 - bias_ref).abs().max().item()
            assert berr <= 0.04 * max(1.0, bias_ref.abs().max().item()), berr
        else:
            assert (dbias == 2.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [164, 177])
def test_resident_bwd_bit_repeatable(dev, S):
    """no atomics on dQ / dK / dV and a fixed reduction order of the per-sample bias sums: two calls give the same bits, also with
    another stream's work on the device in between.  (The second stage adds batch slices of those sums onto the output with
    atomics -- attn_bias_reduce_kernel, as before this kernel -- so the final bias gradient is compared to a last-bit tolerance.)"""
    B = 32 if dev.type == "cuda" else 2
    c = _case(dev, B, S, 0.1, 7 + S)
    d1, b1, w1 = _bwd(c, True)
    w1 = w1[:B * 3 * NH * 64].clone()
    if dev.type == "cuda":
        side = torch.cuda.Stream()
        x = torch.randn(2048, 2048, device=dev)
        with torch.cuda.stream(side):
            for _ in range(4):
                x = x @ x.T / 2048.0
            other = _case(dev, B, 112, 0.1, 3)
            _bwd(other, True, stream=side.cuda_stream)
        d2, b2, w2 = _bwd(c, True)               # on the current stream while the side stream may still be busy
        torch.cuda.synchronize()
    else:
        _bwd(_case(dev, B, 112, 0.1, 3), True)
        d2, b2, w2 = _bwd(c, True)
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))
    assert torch.equal(w1.view(torch.int32), w2[:B * 3 * NH * 64].view(torch.int32))
    assert (b1 - b2).abs().max().item() <= 1e-5 * max(1.0, b1.abs().max().item())
