"""Threshold vs shared-key decryption cost, config #2 ring, k simulated
clients on one GPU — the decrypt sequence SequentialFL runs per round, timed
with device syncs, plus the per-launch breakdown of one party's share."""
import sys, os, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hefl.config import HEConfig
from hefl.he.ckks import CKKSContext, CtxtTensor

K = int(sys.argv[1]) if len(sys.argv) > 1 else 2
SB = 16

def t(fn, iters=50):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, out

cfg = HEConfig(m=8192, scale_bits=40, q_bits=(60, 40), seed=1)
nw = 222_722
ctx = CKKSContext(cfg, device="cuda")
be = ctx.backend
vecs = [torch.randn(nw, device="cuda") for _ in range(K)]

def aggregate(pk):
    agg = None
    for v in vecs:
        ct = ctx.encrypt_tensor(v, pk)
        agg = ct if agg is None else CtxtTensor(agg.data + ct.data, agg.scale, agg.count)
    ctx.modreduce_tensor_(agg)
    return ctx.rescale_tensor(ctx.mul_scalar_tensor(agg, 1.0 / K))

# shared key
kp = ctx.keygen()
ms_agg, avg = t(lambda: aggregate(kp.pk))
ms_dec, out_s = t(lambda: ctx.decrypt_tensor(avg, kp.sk))
print(f"shared   : k={K} encrypt+aggregate {ms_agg:.3f} ms | decrypt {ms_dec:.3f} ms "
      f"| fedavg total {ms_agg + ms_dec:.3f} ms")

# threshold key
a = ctx.sample_crp()
shares = [ctx.keygen_share(a, i) for i in range(K)]
pk = ctx.combine_pk(torch.stack([s.b_share for s in shares]).sum(0), a)
ms_agg_t, avg = t(lambda: aggregate(pk))

def thr_decrypt():
    acc = None
    for i, s in enumerate(shares):
        h = ctx.partial_decrypt_tensor(avg, s.sk_share, SB, lead=i == 0)
        acc = h if acc is None else acc.add_(h)
    return ctx.combine_shares_tensor(acc, avg.scale, avg.count)

ms_thr, out_t = t(thr_decrypt)
mean = torch.stack(vecs).mean(0)
print(f"threshold: k={K} encrypt+aggregate {ms_agg_t:.3f} ms | decrypt {ms_thr:.3f} ms "
      f"| fedavg total {ms_agg_t + ms_thr:.3f} ms | max err {(out_t - mean).abs().max().item():.2e}")

# one party's share, launch by launch
B, Lc, n = avg.data.shape[0], avg.level, ctx.n
ms_bits, bits = t(lambda: ctx._draw_bits((B, n)))
ms_ucr, e = t(lambda: be.uniform_center_rns(bits, SB, Lc))
ms_ntt, e_hat = t(lambda: be.ntt_all_(e))
ms_pd, h = t(lambda: be.pdec_share(avg.data, shares[0].sk_share, e_hat, True))
ms_share, _ = t(lambda: ctx.partial_decrypt_tensor(avg, shares[0].sk_share, SB, True))
lazy = h * K
ms_comb, _ = t(lambda: ctx.combine_shares_tensor(lazy.clone(), avg.scale, avg.count))
print(f"one share: B={B} Lc={Lc} | randint {ms_bits:.3f} | uniform_center_rns {ms_ucr:.3f} "
      f"| ntt_limbs {ms_ntt:.3f} | pdec_share {ms_pd:.3f} | whole share {ms_share:.3f} ms")
print(f"combine (clone + modreduce + decode): {ms_comb:.3f} ms")
print(f"noise sampling + NTT share of one party's share: "
      f"{(ms_bits + ms_ucr + ms_ntt) / (ms_bits + ms_ucr + ms_ntt + ms_pd):.0%}")
