"""conv_bwd_pair (dgrad + wgrad of one small conv in a single launch) against
the separate conv2d_dgrad / conv2d_wgrad launches and a float64 reference,
plus the epoch-graph run with the switch (HEFL_CONV_BWD_PAIR) on and off.

The paired kernel runs the stand-alone kernels' own tile bodies, so dx (one
store per element) is compared bit for bit, and dw too wherever the wgrad is
a single pixel chunk. With several chunks dw is summed by fp32 atomics in
both paths, so it is held to the project's float64 rule
(tests/test_gpu_head_xent.py): e_pair <= 2 * e_separate + 1e-6 * max|ref|.
"""
import pytest
import torch

import hefl
from hefl.ops import functional as Fx

pytestmark = pytest.mark.gpu

# (N, H, W, C, Kout, pad): 3x3 conv, H/W the conv INPUT extent
SHAPES = [
    pytest.param((32, 13, 13, 16, 32, 0), id="cnn2-conv2"),
    pytest.param((1, 5, 5, 16, 8, 0), id="one-dgrad-tile-kout8"),
    pytest.param((2, 7, 9, 16, 32, 0), id="non-square-m-tail"),
    pytest.param((3, 6, 6, 24, 16, 0), id="c24-four-col-tiles"),
    pytest.param((1, 5, 5, 16, 8, 1), id="pad1-dgrad-gather"),
]


def _bf(t):
    return t.float().to(torch.bfloat16)


def _case(shape):
    N, H, W, C, K, pad = shape
    OH, OW = H + 2 * pad - 2, W + 2 * pad - 2
    g = torch.Generator().manual_seed(4321 + N * 13 + C + K + pad)
    dy = _bf(torch.randn(N, OH, OW, K, generator=g))
    w = _bf(torch.randn(K, 3, 3, C, generator=g) * 0.2)
    x = _bf(torch.randn(N, H, W, C, generator=g))
    return dy.cuda(), w.cuda(), x.cuda()


def _dw_ref(dy, x, K, C, pad):
    xn = x.double().cpu().permute(0, 3, 1, 2)
    dyn = dy.double().cpu().permute(0, 3, 1, 2)
    dwn = torch.nn.grad.conv2d_weight(xn, (K, C, 3, 3), dyn, padding=pad)
    return dwn.permute(0, 2, 3, 1).contiguous()


def _check_dw(dw, dw_sep, ref, single_chunk):
    if single_chunk:
        assert torch.equal(dw, dw_sep)
        return
    scale = ref.abs().max().item()
    e_p = (dw.double().cpu() - ref).abs().max().item()
    e_s = (dw_sep.double().cpu() - ref).abs().max().item()
    print(f"dw: e_pair={e_p:.4g} e_separate={e_s:.4g} max|ref|={scale:.4g}")
    assert e_p <= 2 * e_s + 1e-6 * scale, (e_p, e_s, scale)


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_bwd_pair_vs_separate(shape):
    N, H, W, C, K, pad = shape
    C_ = hefl.load_extension()
    dy, w, x = _case(shape)
    assert Fx.conv_bwd_pair_ok(dy, w, pad, H, W)
    dx_s = C_.conv2d_dgrad(dy, w, 1, H, W, pad)
    dw_s = C_.conv2d_wgrad(dy, x, 1, 3, 3, pad)
    dx, dw = C_.conv_bwd_pair(dy, w, x, 3, 3, pad, H, W)
    torch.cuda.synchronize()
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
    assert dw.shape == (K, 3, 3, C) and dw.dtype == torch.float32
    assert torch.equal(dx, dx_s)
    KK = N * dy.shape[1] * dy.shape[2]
    _check_dw(dw, dw_s, _dw_ref(dy, x, K, C, pad), single_chunk=KK <= 128)


@pytest.mark.parametrize("shape", [
    pytest.param((32, 13, 13, 16, 32, 0), id="cnn2-conv2-31-chunks"),
    pytest.param((2, 7, 9, 16, 32, 0), id="single-chunk"),
])
def test_conv_bwd_pair_gkey_consume_and_clear(shape):
    """Epoch-graph contract: with a gkey the multi-chunk dw accumulates into
    the persistent grad buffer, which the captured Adam zeroes after reading.
    Call, clear as Adam would, call again: the second result must still be
    one gradient (a double accumulation or a stale buffer shows here)."""
    N, H, W, C, K, pad = shape
    C_ = hefl.load_extension()
    dy, w, x = _case(shape)
    gkey = 0x5EED0000 + N * 1000 + H
    ref = _dw_ref(dy, x, K, C, pad)
    dw_s = C_.conv2d_wgrad(dy, x, 1, 3, 3, pad)
    dx1, dw1 = C_.conv_bwd_pair(dy, w, x, 3, 3, pad, H, W, gkey=gkey)
    first = dw1.clone()
    dw1.zero_()
    dx2, dw2 = C_.conv_bwd_pair(dy, w, x, 3, 3, pad, H, W, gkey=gkey)
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx2)
    KK = N * dy.shape[1] * dy.shape[2]
    _check_dw(first, dw_s, ref, single_chunk=KK <= 128)
    _check_dw(dw2, dw_s, ref, single_chunk=KK <= 128)
    dw2.zero_()  # leave the buffer as the next user expects it


def test_conv_bwd_pair_past_envelope_runs_separate_launches():
    """Batch 64 of the conv2 shape: 169 dgrad tiles + 183 wgrad blocks is more
    than one block per CU, so the wrapper runs the two stand-alone launches."""
    shape = (64, 13, 13, 16, 32, 0)
    N, H, W, C, K, pad = shape
    C_ = hefl.load_extension()
    dy, w, x = _case(shape)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 169 + 183 > cus
    assert not Fx.conv_bwd_pair_ok(dy, w, pad, H, W)
    dx, dw = C_.conv_bwd_pair(dy, w, x, 3, 3, pad, H, W)
    assert torch.equal(dx, C_.conv2d_dgrad(dy, w, 1, H, W, pad))
    dw_s = C_.conv2d_wgrad(dy, x, 1, 3, 3, pad)
    _check_dw(dw, dw_s, _dw_ref(dy, x, K, C, pad), single_chunk=False)


def test_conv_bwd_pair_autograd_switch(monkeypatch):
    """_ConvReluPoolFn.backward with the switch on and off: same dx bit for
    bit on the workload's conv2, dw within the float64 rule."""
    N, H, W, C, K = 32, 13, 13, 16, 32
    C_ = hefl.load_extension()
    g = torch.Generator().manual_seed(77)
    x0 = _bf(torch.randn(N, H, W, C, generator=g)).cuda()
    w0 = _bf(torch.randn(K, 3, 3, C, generator=g) * 0.2).cuda()
    b0 = (torch.randn(K, generator=g) * 0.1).cuda()
    p, idx, ch, cw = C_.conv2d_relu_pool_fwd(x0, w0, b0, 0)
    dy = _bf(torch.randn(*p.shape, generator=g)).cuda()
    dym, _ = C_.pool_relu_bias_bwd(dy, idx, p, ch, cw)
    ref = _dw_ref(dym, x0, K, C, 0)

    def run(on):
        monkeypatch.setattr(Fx, "_CONV_BWD_PAIR", on)
        x = x0.clone().requires_grad_(True)
        w = w0.float().requires_grad_(True)
        b = b0.clone().requires_grad_(True)
        y = Fx.conv_relu_pool(x, w, b, 0)
        assert torch.equal(y, p)
        y.backward(dy)
        torch.cuda.synchronize()
        return x.grad, w.grad

    dx1, dw1 = run(True)
    dx0, dw0 = run(False)
    assert torch.equal(dx1, dx0)
    _check_dw(dw1, dw0, ref, single_chunk=False)


def test_conv_bwd_epoch_graph_capture_and_replay(monkeypatch):
    """CNN2 client, 80-sample shard at batch 32 through the epoch graph with
    the pairing on: finite loss, every parameter moved, and a second identical
    client with it off ends within the bound the existing GPU op tests use
    (max-norm, 1e-3 of the tensor's scale)."""
    from hefl.config import preset
    from hefl.fl.client import LocalClient

    def run(on):
        monkeypatch.setattr(Fx, "_CONV_BWD_PAIR", on)
        cfg = preset("config2")
        cfg.fl.n_clients = 1
        cfg.fl.samples_per_client = 80
        cfg.train.hip_graphs = True
        c = LocalClient(cfg, 0, device="cuda:0")
        w0 = [p.detach().clone() for p in c.model.parameters()]
        stats = c.local_train(epochs=1)
        assert c._ep_ent["steps"] == 3 and c._ep_ent["n"] == 80
        torch.cuda.synchronize()
        return stats, w0, [p.detach().clone() for p in c.model.parameters()]

    stats, w0, w_on = run(True)
    assert torch.isfinite(torch.tensor(stats.train_loss))
    for a, b in zip(w0, w_on):
        assert torch.isfinite(b).all()
        assert not torch.equal(a, b), "a parameter did not change"
    _, _, w_off = run(False)
    for a, b in zip(w_on, w_off):
        scale = b.abs().max().item() + 1e-8
        err = (a - b).abs().max().item()
        print(f"shape {tuple(b.shape)}: err={err:.4g} scale={scale:.4g}")
        assert err < 1e-3 * scale, (tuple(b.shape), err, scale)
