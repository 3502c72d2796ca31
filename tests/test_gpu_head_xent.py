"""Fused classifier tail (head_xent_fwd / head_xent_bwd) and the paired
dense backward launch (linear_bwd_pair) against the composed GPU ops and a
float64 CPU reference built with the composed path's rounding points."""
import pytest
import torch

import hefl
from hefl.ops import functional as Fx

pytestmark = pytest.mark.gpu

OUT_NAMES = ("loss", "logits", "dx", "dW1", "db1", "dW2", "db2")


def _bf(t):
    """Round to bf16, return as float64 (the rounding points of the path)."""
    return t.float().to(torch.bfloat16).double()


def _bf16_ulp(v):
    """bf16 ulp at |v| (8 significand bits)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def _ref_forward(x, w1, b1, w2, b2):
    h1 = _bf(torch.relu(x @ w1.t() + b1))
    logits = _bf(h1 @ w2.t() + b2)
    return h1, logits


def _top2_gap_ok(logits):
    top = logits.topk(2, dim=-1).values
    gap = top[:, 0] - top[:, 1]
    ulp = _bf16_ulp(torch.maximum(top[:, 0].abs(), top[:, 1].abs()))
    return gap > 4 * ulp


def _draw(M, K, H, C, seed):
    """bf16-exact inputs (as float64) whose reference logits have a top-2 gap
    of more than 4 bf16 ulps in every row: rows that miss it are redrawn on
    the CPU (rows are independent in the forward), so an argmax tie can
    neither hide nor fake an acc_correct failure."""
    g = torch.Generator().manual_seed(seed)
    x = _bf(torch.randn(M, K, generator=g))
    w1 = _bf(torch.randn(H, K, generator=g) / K ** 0.5)
    b1 = (torch.randn(H, generator=g) * 0.1).float().double()
    w2 = _bf(torch.randn(C, H, generator=g) * 2.0 / H ** 0.5)
    b2 = (torch.randn(C, generator=g) * 0.1).float().double()
    for _ in range(200):
        _, logits = _ref_forward(x, w1, b1, w2, b2)
        bad = ~_top2_gap_ok(logits)
        if not bad.any():
            break
        x[bad] = _bf(torch.randn(int(bad.sum()), K, generator=g))
    _, logits = _ref_forward(x, w1, b1, w2, b2)
    # half the labels hit the reference argmax so acc_correct is non-trivial
    y = torch.randint(0, C, (M,), generator=g)
    hit = torch.arange(M) % 2 == 0
    y[hit] = logits.argmax(-1)[hit]
    return x, w1, b1, w2, b2, y


def _reference(x, w1, b1, w2, b2, y, dloss):
    M, C = x.shape[0], w2.shape[0]
    h1, logits = _ref_forward(x, w1, b1, w2, b2)
    p = torch.softmax(logits, -1)
    loss = -torch.log(p[torch.arange(M), y]).mean()
    onehot = torch.nn.functional.one_hot(y, C).double()
    dl = _bf((p - onehot) * (dloss / M))
    db2 = dl.sum(0)
    dW2 = dl.t() @ h1
    dz1 = _bf(dl @ w2) * (h1 > 0).double()
    db1 = dz1.sum(0)
    dx = _bf(dz1 @ w1)
    dW1 = dz1.t() @ x
    correct = float((logits.argmax(-1) == y).sum())
    return dict(loss=loss, logits=logits, dx=dx, dW1=dW1, db1=db1, dW2=dW2,
                db2=db2), correct


def _run_gpu(fused, x, w1, b1, w2, b2, y, dloss, monkeypatch):
    monkeypatch.setattr(Fx, "_HEAD_XENT", fused)
    monkeypatch.setattr(Fx, "_LIN_PAIR", fused)
    xg = x.to("cuda", torch.bfloat16).requires_grad_(True)
    ps = [t.float().cuda().requires_grad_(True) for t in (w1, b1, w2, b2)]
    yg = y.cuda()
    acc_loss = torch.zeros((), device="cuda")
    acc_correct = torch.zeros((), device="cuda")
    if fused:
        loss, logits = Fx.dense_head2_xent(xg, *ps, yg, acc_loss, acc_correct)
    else:
        logits = Fx.linear(Fx.linear(xg, ps[0], ps[1], relu=True), ps[2],
                           ps[3], relu=False)
        loss = Fx.softmax_xent(logits, yg, acc_loss, acc_correct)
    loss.backward(gradient=torch.tensor(dloss, device="cuda"))
    out = dict(loss=loss, logits=logits, dx=xg.grad, dW1=ps[0].grad,
               db1=ps[1].grad, dW2=ps[2].grad, db2=ps[3].grad)
    out = {k: v.detach().double().cpu() for k, v in out.items()}
    return out, float(acc_loss), float(acc_correct)


@pytest.mark.parametrize("M,K,H,C,dloss", [
    (32, 800, 64, 10, 0.5),    # config #2 full batch, dloss != 1
    (16, 800, 64, 10, 1.0),    # the real tail batch of a 720-sample shard
    (1, 32, 8, 2, 1.0),
    (5, 40, 24, 3, 0.5),
    (32, 120, 84, 10, 1.0),    # config #3 head: H not a multiple of 8
    (64, 64, 128, 16, 1.0),    # envelope corner
])
def test_head_xent_fused_vs_composed_vs_f64(M, K, H, C, dloss, monkeypatch):
    """For each output, e = max|out - ref| against the float64 reference
    built from the same bf16 inputs and rounding points; require
    e_fused <= 2 * e_composed + 1e-6 * max|ref| (a different fp32 summation
    order can move a bf16-rounded intermediate at most one rounding step
    further than the composed path's own half-ulp error)."""
    x, w1, b1, w2, b2, y = _draw(M, K, H, C, seed=1000 + M + H)
    _, ref_logits = _ref_forward(x, w1, b1, w2, b2)
    assert _top2_gap_ok(ref_logits).all(), "top-2 gap precondition"
    ref, ref_correct = _reference(x, w1, b1, w2, b2, y, dloss)
    assert Fx.head_xent_ok(x.to("cuda", torch.bfloat16), w1, w2)
    fused, f_acc_loss, f_correct = _run_gpu(True, x, w1, b1, w2, b2, y,
                                            dloss, monkeypatch)
    comp, c_acc_loss, c_correct = _run_gpu(False, x, w1, b1, w2, b2, y,
                                           dloss, monkeypatch)
    fails = []
    for name in OUT_NAMES:
        scale = ref[name].abs().max().item()
        e_f = (fused[name] - ref[name]).abs().max().item()
        e_c = (comp[name] - ref[name]).abs().max().item()
        print(f"{name}: e_fused={e_f:.4g} e_composed={e_c:.4g} "
              f"max|ref|={scale:.4g}")
        if not e_f <= 2 * e_c + 1e-6 * scale:
            fails.append((name, e_f, e_c, scale))
    ref_loss = ref["loss"].item()
    e_f = abs(f_acc_loss - ref_loss)
    e_c = abs(c_acc_loss - ref_loss)
    print(f"acc_loss: e_fused={e_f:.4g} e_composed={e_c:.4g}")
    if not e_f <= 2 * e_c + 1e-6 * abs(ref_loss):
        fails.append(("acc_loss", e_f, e_c, abs(ref_loss)))
    assert not fails, fails
    assert f_correct == ref_correct, (f_correct, ref_correct)
    assert c_correct == ref_correct, (c_correct, ref_correct)


@pytest.mark.parametrize("M,K,H,C", [
    (32, 800, 64, 10), (16, 800, 64, 10), (5, 40, 24, 3), (32, 120, 84, 10),
    (64, 64, 128, 16),
])
def test_head_xent_bit_identical_to_composed(M, K, H, C, monkeypatch):
    """The fused kernels keep the composed kernels' MFMA k-order, rounding
    points AND the summation order of the two bias-gradient reductions, so
    every output (and the accumulated stats) equals the composed path's
    bit for bit — the training trajectory cannot move."""
    x, w1, b1, w2, b2, y = _draw(M, K, H, C, seed=2000 + M + H)
    a, a_loss, a_corr = _run_gpu(True, x, w1, b1, w2, b2, y, 0.5, monkeypatch)
    b, b_loss, b_corr = _run_gpu(False, x, w1, b1, w2, b2, y, 0.5,
                                 monkeypatch)
    for name in OUT_NAMES:
        assert torch.equal(a[name], b[name]), name
    assert a_loss == b_loss and a_corr == b_corr


@pytest.mark.parametrize("M,H,C", [(65, 24, 5), (8, 136, 5), (8, 24, 17)])
def test_head_xent_out_of_envelope_is_composed(M, H, C, monkeypatch):
    """One step outside the envelope (M=65, H=136, C=17, each alone) the
    wrapper runs the composed ops unchanged: every output torch.equal."""
    K = 32
    x, w1, b1, w2, b2, y = _draw(M, K, H, C, seed=7)
    assert not Fx.head_xent_ok(x.to("cuda", torch.bfloat16), w1, w2)
    a, a_loss, a_corr = _run_gpu(True, x, w1, b1, w2, b2, y, 1.0, monkeypatch)
    # _LIN_PAIR is bit-identical by construction (checked below), so the
    # composed side runs with both switches off, as before this change
    b, b_loss, b_corr = _run_gpu(False, x, w1, b1, w2, b2, y, 1.0,
                                 monkeypatch)
    for name in OUT_NAMES:
        assert torch.equal(a[name], b[name]), name
    assert a_loss == b_loss and a_corr == b_corr


@pytest.mark.parametrize("M,N,K", [
    (32, 64, 800), (16, 64, 800), (1, 8, 32), (5, 24, 40), (64, 128, 512),
    (70, 10, 33),
])
def test_linear_bwd_pair_bit_identical(M, N, K):
    C_ = hefl.load_extension()
    g = torch.Generator().manual_seed(M * 131 + N)
    dy = torch.randn(M, N, generator=g).to("cuda", torch.bfloat16)
    w = torch.randn(N, K, generator=g).to("cuda", torch.bfloat16)
    x = torch.randn(M, K, generator=g).to("cuda", torch.bfloat16)
    dx, dw = C_.linear_bwd_pair(dy, w, x)
    assert torch.equal(dx, C_.linear_dgrad(dy, w))
    assert torch.equal(dw, C_.linear_wgrad(dy, x))


def test_head_xent_epoch_graph_capture_and_replay(monkeypatch):
    """CNN2 client, 80-sample shard at batch 32 (two full steps + a 16-row
    tail) through the epoch graph with both switches on: finite loss, every
    parameter moved, and a second identical client with both switches off
    ends within the fused-versus-composed bound the existing GPU op tests
    use (max-norm, 1e-3 of the tensor's scale; tests/test_gpu_ops.py)."""
    from hefl.config import preset
    from hefl.fl.client import LocalClient

    def run(on):
        monkeypatch.setattr(Fx, "_HEAD_XENT", on)
        monkeypatch.setattr(Fx, "_LIN_PAIR", on)
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
