"""fc1's whole-K panel forward (linear_panel_kernel) against the kernel it
stands in for, linear_splitk_kernel<1>. Same MFMA chain, same operand slots,
same rounding points, so every comparison is torch.equal."""
import pytest
import torch

import hefl
from hefl.ops import functional as Fx

pytestmark = pytest.mark.gpu


def _draw(shape, g):
    """Seeded randn rounded to bf16, every 7th element an exact zero
    (negatives come with randn)."""
    t = torch.randn(*shape, generator=g)
    t.view(-1)[::7] = 0.0
    return t.to(torch.bfloat16)


def _fwd_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (_draw((M, K), g).cuda(), _draw((N, K), g).cuda(),
            torch.randn(N, generator=g).cuda())


FWD_SHAPES = [
    (32, 64, 800),    # the workload
    (16, 64, 800),    # the epoch's tail batch
    (1, 8, 32),
    (5, 24, 40),
    (33, 16, 64),
    (64, 128, 512),
    (32, 16, 1024),   # envelope edge (dynamic LDS above the default limit)
    (32, 64, 1056),   # outside: split-K either way
    (7, 20, 100),     # K % 8 != 0: the 2-byte-load instantiation
]


@pytest.mark.parametrize("M,N,K", FWD_SHAPES)
def test_linear_fwd_panel_bit_identical(M, N, K):
    C_ = hefl.load_extension()
    x, w, b = _fwd_case(M, N, K, seed=M * 1009 + N * 31 + K)
    inside = M <= 64 and K <= 1024
    assert Fx.linear_fwd_panel_ok(x, w) == inside
    empty = torch.empty(0, device="cuda")
    for bias in (b, empty):
        for relu in (False, True):
            new = C_.linear_fwd(x, w, bias, relu)               # default: on
            old = C_.linear_fwd(x, w, bias, relu, panel=False)
            assert new.shape == (M, N) and new.dtype == torch.bfloat16
            assert torch.equal(new, old), (bias.numel(), relu)


def test_linear_fwd_panel_unaligned_base():
    """A contiguous x whose base is 2 bytes past a 16-byte boundary: still
    inside the envelope (2-byte loads), still the same bits."""
    C_ = hefl.load_extension()
    M, N, K = 32, 64, 800
    x, w, b = _fwd_case(M, N, K, seed=5)
    buf = torch.zeros(M * K + 8, dtype=torch.bfloat16, device="cuda")
    xo = buf[1:1 + M * K].view(M, K)
    xo.copy_(x)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 2
    assert Fx.linear_fwd_panel_ok(xo, w)
    new = C_.linear_fwd(xo, w, b, True)
    assert torch.equal(new, C_.linear_fwd(xo, w, b, True, panel=False))
    assert torch.equal(new, C_.linear_fwd(x, w, b, True))


def test_linear_fwd_panel_predicate_sides():
    x, w, _ = _fwd_case(64, 16, 1024, seed=1)
    assert Fx.linear_fwd_panel_ok(x, w)
    x, w, _ = _fwd_case(65, 16, 64, seed=2)
    assert not Fx.linear_fwd_panel_ok(x, w)      # M > 64: the tiled GEMM
    x, w, _ = _fwd_case(8, 16, 1032, seed=3)
    assert not Fx.linear_fwd_panel_ok(x, w)      # K > 1024: split-K


def test_linear_switch_is_honoured(monkeypatch):
    """Fx.linear with HEFL_LIN_FWD_PANEL on and off: same y."""
    x, w, b = _fwd_case(32, 64, 800, seed=11)
    ys = []
    for on in (True, False):
        monkeypatch.setattr(Fx, "_LIN_FWD_PANEL", on)
        ys.append(Fx.linear(x, w.float(), b, relu=True))
    assert torch.equal(ys[0], ys[1])


def _fc1_step(model, x0, labels, on, monkeypatch):
    """h1, dx, dw1 of the workload's classifier tail on fixed inputs."""
    monkeypatch.setattr(Fx, "_LIN_FWD_PANEL", on)
    fc1, fc2 = model.head[-2], model.head[-1]
    x = x0.clone().requires_grad_(True)
    for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias):
        p.grad = None
    h1 = Fx.linear(x0, fc1.weight.detach(), fc1.bias.detach(), relu=True)
    loss, _ = Fx.dense_head2_xent(x, fc1.weight, fc1.bias, fc2.weight,
                                  fc2.bias, labels)
    loss.backward()
    torch.cuda.synchronize()
    return h1, x.grad.clone(), fc1.weight.grad.clone()


def test_epoch_graph_and_fc1_step_switch(monkeypatch):
    """CNN2 client, 80-sample shard at batch 32 (two full steps and a 16-row
    tail) through the epoch graph with the switch on, then off:
    finite loss, every parameter moved. Whole-run parameters are not compared
    bit for bit (the conv backward's fp32 atomics arrive in any order);
    instead fc1's h1, dx and dw1 of one step on fixed inputs, at 32 and at
    16 rows, are torch.equal between the two settings."""
    from hefl.config import preset
    from hefl.fl.client import LocalClient

    def run(on):
        monkeypatch.setattr(Fx, "_LIN_FWD_PANEL", on)
        cfg = preset("config2")
        cfg.fl.n_clients = 1
        cfg.fl.samples_per_client = 80
        cfg.train.hip_graphs = True
        c = LocalClient(cfg, 0, device="cuda:0")
        w0 = [p.detach().clone() for p in c.model.parameters()]
        stats = c.local_train(epochs=1)
        assert c._ep_ent["steps"] == 3 and c._ep_ent["n"] == 80
        torch.cuda.synchronize()
        assert torch.isfinite(torch.tensor(stats.train_loss))
        for a, p in zip(w0, c.model.parameters()):
            assert torch.isfinite(p).all()
            assert not torch.equal(a, p.detach()), "a parameter did not change"
        return c

    c = run(True)
    run(False)
    K = c.model.head[-2].weight.shape[1]
    assert K == 800
    g = torch.Generator().manual_seed(77)
    for M in (32, 16):
        x0 = torch.relu(_draw((M, K), g).float()).to(torch.bfloat16).cuda()
        labels = torch.randint(0, 10, (M,), generator=g).cuda()
        assert Fx.head_xent_ok(x0, c.model.head[-2].weight,
                               c.model.head[-1].weight)
        on = _fc1_step(c.model, x0, labels, True, monkeypatch)
        off = _fc1_step(c.model, x0, labels, False, monkeypatch)
        for name, a, b in zip(("h1", "dx", "dw1"), on, off):
            assert a.abs().max().item() > 0, name
            assert torch.equal(a, b), (M, name)
