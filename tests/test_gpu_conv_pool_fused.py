"""conv2d_relu_pool_fwd (2x2 max-pool fused into the conv forward epilogue)
against the composed conv2d_fwd(relu) -> maxpool2x2_fwd pair.

The forward comparison is bit-exact on purpose: a pixel's fp32 accumulator
does not depend on which tile row it occupies (same k order, same MFMA), the
bias/ReLU/bf16 rounding is the same code, rounding is monotone, and the
first-maximum-wins compare chain is the one maxpool_fwd_oct_kernel runs on
the rounded values. So `p` and `idx` must be `torch.equal`, ties included.
"""
import os

import pytest
import torch

import hefl
from hefl.ops import functional as Fx

pytestmark = pytest.mark.gpu

# (N, H, W, C, Kout, k, pad, env) — the smallest shapes at which each piece
# of the fused path can go wrong
FWD_SHAPES = [
    # generic <64,16>: one partial M tile, odd 5x5 output (row+col dropped)
    pytest.param((2, 7, 7, 1, 16, 3, 0), None, id="g16-partial-odd"),
    # generic <64,16>: column tail (Kout=6), 5x5 taps, scalar-gather branch
    pytest.param((2, 9, 8, 3, 6, 5, 0), None, id="g16-coltail-5x5"),
    # generic <64,16>: cnn2 block 1, many tiles
    pytest.param((4, 28, 28, 1, 16, 3, 0), None, id="g16-cnn2-block1"),
    # generic <64,64>: C % 8 != 0 with Kout > 16
    pytest.param((2, 8, 8, 3, 24, 3, 0), None, id="g64-c3"),
    # glds: fewer than 16 blocks, xcd_remap is the identity
    pytest.param((2, 8, 8, 16, 32, 3, 0), None, id="glds-small"),
    # glds: cnn2 block 2, odd 11 -> 5, 50 tiles, remap active, last tile full
    pytest.param((32, 13, 13, 16, 32, 3, 0), None, id="glds-cnn2-block2"),
    # glds: M tail inside the last tile
    pytest.param((5, 13, 13, 16, 32, 3, 0), None, id="glds-mtail"),
    # glds: KK=72 (K tail) and a column tail
    pytest.param((2, 8, 8, 8, 24, 3, 0), None, id="glds-ktail-coltail"),
    # glds: pad-1 halo through the zero scratch, two column tiles
    pytest.param((2, 6, 6, 8, 80, 3, 1), None, id="glds-pad1-2coltiles"),
    # fallback: split-K shape (k_chunks > 1) runs the composed pair
    pytest.param((2, 6, 6, 64, 64, 3, 0), None, id="fallback-splitk"),
    # fallback: direct tiled dispatch runs the composed pair
    pytest.param((4, 20, 20, 32, 32, 3, 0), {"HEFL_TILE3": "2"},
                 id="fallback-tile3"),
]


class _Env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _inputs(shape):
    N, H, W, C, K, ks, _ = shape
    torch.manual_seed(0)
    x = torch.randn(N, H, W, C, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn(K, ks, ks, C, device="cuda") * 0.1).to(torch.bfloat16)
    b = torch.randn(K, device="cuda") * 0.05
    return x, w, b


def _both(C_, x, w, b, pad, env):
    with _Env(env):
        y = C_.conv2d_fwd(x, w, b, 1, True, pad)
        p_ref, idx_ref = C_.maxpool2x2_fwd(y)
        p, idx, oh, ow = C_.conv2d_relu_pool_fwd(x, w, b, pad)
    torch.cuda.synchronize()
    return y, p_ref, idx_ref, p, idx, oh, ow


@pytest.mark.parametrize("shape,env", FWD_SHAPES)
def test_fused_forward_bit_exact(shape, env):
    C_ = hefl.load_extension()
    pad = shape[6]
    x, w, b = _inputs(shape)
    y, p_ref, idx_ref, p, idx, oh, ow = _both(C_, x, w, b, pad, env)
    assert (oh, ow) == (y.shape[1], y.shape[2])
    assert p.shape == p_ref.shape and p.dtype == torch.bfloat16
    assert idx.shape == idx_ref.shape and idx.dtype == torch.uint8
    assert torch.isfinite(p_ref.float()).all()
    assert torch.equal(p, p_ref)
    assert torch.equal(idx, idx_ref)


@pytest.mark.parametrize("shape,env", FWD_SHAPES)
def test_fused_forward_tie_rule(shape, env):
    """Bias -10 on every other channel drives whole windows to 0 after the
    ReLU: the 0-vs-0 ties must resolve to the first cell (idx 0), as in the
    separate pool kernel — the backward scatters by idx."""
    C_ = hefl.load_extension()
    pad = shape[6]
    x, w, b = _inputs(shape)
    b = b.clone()
    b[::2] = -10.0
    y, p_ref, idx_ref, p, idx, _, _ = _both(C_, x, w, b, pad, env)
    assert torch.equal(p, p_ref)
    assert torch.equal(idx, idx_ref)
    N, PH, PW, K = p_ref.shape
    win = y[:, :2 * PH, :2 * PW].reshape(N, PH, 2, PW, 2, K).float()
    dead = win.amax(dim=(2, 4)) == 0  # [N, PH, PW, K]: all four cells are 0
    assert dead.any(), "no all-zero window: the tie rule was not exercised"
    assert (p[dead].float() == 0).all()
    assert (idx[dead] == 0).all()


def _rel_close(a, b, rel):
    # same rule as test_conv_relu_pool_fused_matches_composed: max-norm
    # error scaled to the reference tensor
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    scale = b.abs().max().item() + 1e-8
    err = (a - b).abs().max().item()
    assert err < rel * scale, f"max abs err {err:.4g} vs scale {scale:.4g}"


@pytest.mark.parametrize("shape", [
    (4, 28, 28, 1, 16, 3),    # cnn2 block 1
    (32, 13, 13, 16, 32, 3),  # cnn2 block 2
    (2, 32, 32, 3, 6, 5),     # lenet5 block 1
])
def test_autograd_switch_on_matches_off(shape, monkeypatch):
    """Fx.conv_relu_pool with the fused forward on vs off: outputs equal,
    grads to the rel=1e-3 rule (backward kernels are unchanged; some use
    float atomics)."""
    N, H, W, C, K, ks = shape
    torch.manual_seed(0)
    x = torch.randn(N, H, W, C, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, ks, ks, C, device="cuda") * 0.1
    b = torch.randn(K, device="cuda") * 0.05

    def run(on):
        monkeypatch.setattr(Fx, "_CONV_POOL", on)
        xd = x.clone().requires_grad_(True)
        wd = torch.nn.Parameter(w.clone())
        bd = torch.nn.Parameter(b.clone())
        y = Fx.conv_relu_pool(xd, wd, bd)
        y.float().pow(2).sum().backward()
        return y.detach(), xd.grad, wd.grad, bd.grad

    y1, dx1, dw1, db1 = run(True)
    y0, dx0, dw0, db0 = run(False)
    assert torch.equal(y1, y0)
    _rel_close(dx1, dx0, 1e-3)
    _rel_close(dw1, dw0, 1e-3)
    _rel_close(db1, db0, 1e-3)
