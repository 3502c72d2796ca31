"""CPU contract of the fused classifier tail: `Fx.dense_head2_xent` and
`_SeqCNN.forward_loss` are, on CPU, literally the composed
linear -> linear -> softmax_xent ops — every output bit-identical."""
import torch

from hefl.models import CNN2, RefCNN6
from hefl.models.cnn import _SeqCNN
from hefl.ops import functional as Fx


def _grads(fn, x, params):
    xd = x.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in params]
    loss, logits = fn(xd, *ps)
    loss.backward()
    return [loss.detach(), logits.detach(), xd.grad] + [p.grad for p in ps]


def test_dense_head2_xent_cpu_bit_identical():
    torch.manual_seed(3)
    M, K, H, C = 7, 40, 24, 5
    x = torch.randn(M, K)
    params = [torch.randn(H, K) * 0.1, torch.randn(H) * 0.1,
              torch.randn(C, H) * 0.1, torch.randn(C) * 0.1]
    y = torch.randint(0, C, (M,))

    def fused(xd, w1, b1, w2, b2):
        return Fx.dense_head2_xent(xd, w1, b1, w2, b2, y)

    def composed(xd, w1, b1, w2, b2):
        logits = Fx.linear(Fx.linear(xd, w1, b1, relu=True), w2, b2)
        return Fx.softmax_xent(logits, y), logits

    got = _grads(fused, x, params)
    ref = _grads(composed, x, params)
    assert len(got) == 7  # loss, logits, dx, dW1, db1, dW2, db2
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def _check_forward_loss(model, x, y):
    def run(fn):
        model.zero_grad()
        loss, logits = fn()
        loss.backward()
        return [loss.detach(), logits.detach()] + \
            [p.grad.clone() for p in model.parameters()]

    def composed():
        logits = model(x)
        return Fx.softmax_xent(logits, y), logits

    got = run(lambda: model.forward_loss(x, y))
    ref = run(composed)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_cnn2_forward_loss_equals_composed():
    torch.manual_seed(0)
    m = CNN2((28, 28, 1), 10, seed=1)
    _check_forward_loss(m, torch.randn(6, 28, 28, 1),
                        torch.randint(0, 10, (6,)))


def test_three_dense_head_forward_loss_equals_composed():
    # RefCNN6 at a small input: six conv/pool blocks need >= 190 px to keep
    # one pixel, so 190x190 -> 128 features -> 128 -> 64 -> 2
    torch.manual_seed(1)
    m = RefCNN6((190, 190, 3), 2, seed=2)
    assert len(m.head) == 3
    _check_forward_loss(m, torch.randn(2, 190, 190, 3),
                        torch.randint(0, 2, (2,)))


def test_unqualified_head_forward_loss_equals_composed():
    # single-Dense head: no Dense(relu) -> Dense pair to fuse
    torch.manual_seed(2)
    m = _SeqCNN((12, 12, 1), (4,), 3, (), 3, seed=3)
    assert len(m.head) == 1
    _check_forward_loss(m, torch.randn(5, 12, 12, 1),
                        torch.randint(0, 3, (5,)))
