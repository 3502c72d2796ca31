"""conv1_pool_bwd (first-layer conv->relu->pool backward, bias role + gated
small wgrad in ONE launch) against pool_relu_bias_bwd + conv2d_wgrad on the
same inputs, plus _ConvReluPoolFn.backward with the switch (HEFL_CONV1_BWD)
on and off. p / idx come from a real conv2d_relu_pool_fwd.

dw is atomic-free in both paths (per-chunk slabs, fixed-order slab sum), so
it is compared bit for bit on every shape. db is summed by fp32 atomics in
arrival order in both paths, so it is checked two ways:
- dy on a grid where every fp32 partial sum is exact (bf16 multiples of 2^-6
  with |v| <= 4: at most N*PH*PW*256 <= 2^21 grid units at the workload
  shape, inside fp32's 24 bits) -> db equals the composed path and the
  float64 sum bit for bit whatever the order;
- normal dy -> |db - db64| <= n * 2^-24 * sum|terms| per channel, the fp32
  worst-case summation bound for n terms in any order.
"""
import pytest
import torch

import hefl
from hefl.ops import functional as Fx

pytestmark = pytest.mark.gpu

# (N, H, W, C, Kout, R, pad): H/W the conv INPUT extent, R x R filter
IN_ENVELOPE = {
    # one block per role, kc = 1, direct-store db
    "n2-6x6-k8": (2, 6, 6, 1, 8, 3, 0),
    # conv 5x5: the odd row and column a floor pool drops must stage as zero
    "n1-7x7-k16-odd": (1, 7, 7, 1, 16, 3, 0),
    # KK = 400: kc = 2, chunks of 200 = 128 + a 72-pixel tail
    "n4-12x12-k16-kc2-tail": (4, 12, 12, 1, 16, 3, 0),
    # noct 4 / FM 2, conv 7x7 odd
    "n3-9x9-k32": (3, 9, 9, 1, 32, 3, 0),
    # noct 8 / FM 4, 7 bias blocks (db by global atomics), kc = 4
    "n8-12x12-k64": (8, 12, 12, 1, 64, 3, 0),
    # 4x4 filter, C = 1: NN = 16 fills the MFMA B columns
    "n2-9x9-k16-r4": (2, 9, 9, 1, 16, 4, 0),
    # 3x3 with pad = 1: x patches cross the border
    "n2-6x6-k16-pad1": (2, 6, 6, 1, 16, 3, 1),
    # the workload's own layer: 43 + 85 blocks
    "cnn2-conv1": (32, 28, 28, 1, 16, 3, 0),
}
OUTSIDE = {
    # R*S*C = 144 > 16: conv2d_wgrad does not take the small tile
    "rsc-144": (2, 7, 7, 16, 16, 3, 0),
    # 169 bias blocks + 338 wgrad chunks: more than one block per CU
    "past-one-block-per-cu": (128, 28, 28, 1, 16, 3, 0),
}
ALL = {**IN_ENVELOPE, **OUTSIDE}

_CACHE = {}


def _bf(t):
    return t.float().to(torch.bfloat16)


def _case(name):
    """Inputs and the composed path's results, computed once per shape and
    left unchanged. Bias: every third channel far negative (each window of
    theirs pools to p == 0), the rest positive; channel 1 has zero weights,
    so its conv output is its bias everywhere and the four cells of every
    window of its tie at a positive maximum."""
    if name in _CACHE:
        return _CACHE[name]
    N, H, W, C, K, R, pad = ALL[name]
    C_ = hefl.load_extension()
    g = torch.Generator().manual_seed(9000 + N * 131 + H * 17 + K + R + pad)
    x = _bf(torch.randn(N, H, W, C, generator=g))
    w = _bf(torch.randn(K, R, R, C, generator=g) * 0.5)
    w[1] = 0
    b = torch.rand(K, generator=g) * 0.5 + 0.25
    b[::3] = -100.0
    x, w, b = x.cuda(), w.cuda(), b.cuda()
    p, idx, ch, cw = C_.conv2d_relu_pool_fwd(x, w, b, pad)
    assert (ch, cw) == (H + 2 * pad - R + 1, W + 2 * pad - R + 1)
    PH, PW = p.shape[1], p.shape[2]
    # what the inputs are meant to contain
    assert (p[..., 0] == 0).all()
    y = C_.conv2d_fwd(x, w, b, 1, True, pad)[:, : 2 * PH, : 2 * PW]
    win = y.float().reshape(N, PH, 2, PW, 2, K)
    tied = (win.amax((2, 4)) == win.amin((2, 4))) & (p.float() > 0)
    assert tied[..., 1].all(), "channel 1's windows do not tie above zero"
    # dy: exact grid (multiples of 2^-6, |v| <= 4) and normal
    dy_grid = _bf(torch.randint(-256, 257, p.shape, generator=g).float()
                  / 64).cuda()
    dy_norm = _bf(torch.randn(p.shape, generator=g)).cuda()
    case = dict(x=x, p=p, idx=idx, ch=ch, cw=cw, R=R, pad=pad, K=K,
                n_terms=N * PH * PW)
    for tag, dy in (("grid", dy_grid), ("norm", dy_norm)):
        dym, db = C_.pool_relu_bias_bwd(dy, idx, p, ch, cw)
        dw = C_.conv2d_wgrad(dym, x, 1, R, R, pad)
        terms = dy.double() * (p.float() > 0)
        case[tag] = dict(dy=dy, dw=dw, db=db,
                         db64=terms.sum((0, 1, 2)),
                         dbabs=terms.abs().sum((0, 1, 2)))
    torch.cuda.synchronize()
    _CACHE[name] = case
    return case


def _fused(case, dy, **keys):
    C_ = hefl.load_extension()
    dw, db = C_.conv1_pool_bwd(dy, case["idx"], case["p"], case["x"],
                               case["R"], case["R"], case["pad"], case["ch"],
                               case["cw"], **keys)
    torch.cuda.synchronize()
    return dw, db


def _ok(case, dy):
    return hefl.load_extension().conv1_pool_bwd_ok(
        dy, case["x"], case["R"], case["R"], case["pad"], case["ch"],
        case["cw"])


def _check(case, tag):
    ref = case[tag]
    dw, db = _fused(case, ref["dy"])
    assert dw.shape == ref["dw"].shape and dw.dtype == torch.float32
    assert db.shape == (case["K"],) and db.dtype == torch.float32
    assert torch.equal(dw, ref["dw"])
    err = (db.double() - ref["db64"]).abs()
    if tag == "grid":
        assert torch.equal(db, ref["db"])
        assert torch.equal(db.double(), ref["db64"])
    else:
        bound = case["n_terms"] * 2.0 ** -24 * ref["dbabs"]
        print(f"db: max err={err.max().item():.4g} "
              f"min slack={(bound - err).min().item():.4g}")
        assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("name", list(IN_ENVELOPE))
def test_conv1_pool_bwd_exact_grid(name):
    case = _case(name)
    assert _ok(case, case["grid"]["dy"])
    _check(case, "grid")


@pytest.mark.parametrize("name", list(IN_ENVELOPE))
def test_conv1_pool_bwd_normal_dy(name):
    case = _case(name)
    _check(case, "norm")


@pytest.mark.parametrize("name", list(OUTSIDE))
def test_conv1_pool_bwd_outside_envelope_runs_composed_launches(name):
    case = _case(name)
    N, H, W, C, K, R, pad = ALL[name]
    if name == "past-one-block-per-cu":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert 169 + 338 > cus
    assert not _ok(case, case["grid"]["dy"])
    _check(case, "grid")
    _check(case, "norm")


def test_conv1_pool_bwd_bkey_consume_and_clear():
    """Epoch-graph contract at the workload's layer: with a bkey the
    multi-block db accumulates into the persistent grad buffer, which the
    captured Adam zeroes after reading. Call, clear as Adam would, call
    again: the second result must still be one gradient."""
    case = _case("cnn2-conv1")
    ref = case["grid"]
    bkey = 0x5EED1000
    dw1, db1 = _fused(case, ref["dy"], bkey=bkey, wkey=bkey + 1)
    first = db1.clone()
    db1.zero_()
    dw2, db2 = _fused(case, ref["dy"], bkey=bkey, wkey=bkey + 1)
    assert torch.equal(first, ref["db"]) and torch.equal(db2, ref["db"])
    assert torch.equal(dw1, ref["dw"]) and torch.equal(dw2, ref["dw"])
    db2.zero_()  # leave the buffer as the next user expects it


def test_conv1_bwd_autograd_switch(monkeypatch):
    """Fx.conv_relu_pool backward on the workload's first layer (x needs no
    gradient) with the switch on and off: equal dw, and equal db on the
    exact grid."""
    N, H, W, C, K, R, pad = ALL["cnn2-conv1"]
    g = torch.Generator().manual_seed(31)
    x0 = _bf(torch.rand(N, H, W, C, generator=g)).cuda()
    w0 = _bf(torch.randn(K, R, R, C, generator=g) * 0.3).cuda()
    b0 = (torch.randn(K, generator=g) * 0.1).cuda()
    dy = _bf(torch.randint(-256, 257, (N, 13, 13, K), generator=g).float()
             / 64).cuda()

    def run(on):
        monkeypatch.setattr(Fx, "_CONV1_BWD", on)
        w = w0.float().requires_grad_(True)
        b = b0.clone().requires_grad_(True)
        y = Fx.conv_relu_pool(x0, w, b, pad)
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), w.grad, b.grad

    y1, dw1, db1 = run(True)
    y0, dw0, db0 = run(False)
    assert torch.equal(y1, y0)
    assert dw1.abs().max().item() > 0
    assert torch.equal(dw1, dw0)
    assert torch.equal(db1, db0)
