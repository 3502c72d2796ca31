"""Real vs complex packing on one GPU, BASELINE configs #2, #3 and #5: the
ciphertext count and bytes of one client's upload, and the device time of the
three HE phases of a FedAvg round — encrypt, homomorphic aggregate (modreduce
+ ct x 1/n + rescale; ct x ct + relinearise at config #3, which runs the
encrypted denominator) and decrypt — plus, at config #2, the threshold
decryption of k = 2 and k = 8 parties.

Timing as in bench_he.py: a warm-up call, then a host clock around N calls
ending in a device synchronise. N is sized so that a window lasts about a
quarter of a second; every figure is the median of REPS windows, taken
alternately for the two packings, with the lowest and highest window beside it
as the run-to-run spread."""
import sys, os, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses
import statistics

import numpy as np
import torch
from hefl.config import HEConfig
from hefl.he.ckks import CKKSContext, Ciphertext, CtxtTensor

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WINDOW_S = 0.25
SB = 16


def window(fn, iters):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def iters_for(fn):
    ms = window(fn, 3)
    return int(min(500, max(10, WINDOW_S * 1e3 / ms)))


class Case:
    """One (config, packing): its context, keys and the phases to time."""

    def __init__(self, cfg, nw, packing, encrypted_denom, thresholds):
        self.ctx = ctx = CKKSContext(
            dataclasses.replace(cfg, packing=packing), device="cuda")
        self.kp = kp = ctx.keygen()
        self.vec = vec = torch.randn(nw, device="cuda",
                                     generator=torch.Generator("cuda").manual_seed(1))
        ct = ctx.encrypt_tensor(vec, kp.pk)
        self.B, self.bytes = ct.data.shape[0], ct.data.numel() * 8
        self.lazy = CtxtTensor(ct.data * 3, ct.scale, ct.count, ct.packing)
        if encrypted_denom:
            rlk = ctx.relin_keygen(kp.sk)
            denom = ctx.encrypt(ctx.encode(np.full(ctx.slots, 0.125)), kp.pk)

            def divide(c):
                prod = ctx.mul_ct(Ciphertext(c.data, c.scale), denom, rlk)
                return ctx.rescale_tensor(
                    CtxtTensor(prod.data, prod.scale, c.count, c.packing))
        else:
            def divide(c):
                return ctx.rescale_tensor(ctx.mul_scalar_tensor(c, 0.125))
        self.avg = avg = divide(ctx.modreduce_tensor_(
            CtxtTensor(ct.data.clone(), ct.scale, ct.count, ct.packing)))
        self.err = (ctx.decrypt_tensor(avg, kp.sk) - vec / 8).abs().max().item()
        self.phases = {
            "encrypt": lambda: ctx.encrypt_tensor(vec, kp.pk),
            "aggregate": lambda: divide(ctx.modreduce_tensor_(self.lazy)),
            "decrypt": lambda: ctx.decrypt_tensor(avg, kp.sk),
        }
        for k in thresholds:
            a = ctx.sample_crp()
            shares = [ctx.keygen_share(a, i) for i in range(k)]

            def thr(shares=shares):
                acc = None
                for i, s in enumerate(shares):
                    h = ctx.partial_decrypt_tensor(avg, s.sk_share, SB,
                                                   lead=i == 0)
                    acc = h if acc is None else acc.add_(h)
                return ctx.combine_shares_tensor(acc, avg.scale, avg.count,
                                                 packing=avg.packing)
            self.phases[f"threshold decrypt k={k}"] = thr
        self.iters = {p: iters_for(fn) for p, fn in self.phases.items()}
        self.ms = {p: [] for p in self.phases}


CONFIGS = [
    ("config2", HEConfig(m=8192, scale_bits=40, q_bits=(60, 40), seed=1), 222_722, False, (2, 8)),
    ("config3", HEConfig(m=16384, scale_bits=40, q_bits=(60, 40, 40), seed=1), 62_006, True, ()),
    ("config5", HEConfig(m=32768, scale_bits=40, q_bits=(60, 40, 40, 40), seed=1), 11_181_642, False, ()),
]

print(f"# {REPS} alternated windows per figure; ms = median [lowest .. highest]")
for name, cfg, nw, enc_denom, thresholds in CONFIGS:
    cases = {p: Case(cfg, nw, p, enc_denom, thresholds)
             for p in ("real", "complex")}
    for _ in range(REPS):
        for p in ("real", "complex"):          # alternate the two packings
            c = cases[p]
            for phase, fn in c.phases.items():
                c.ms[phase].append(window(fn, c.iters[phase]))
    r, x = cases["real"], cases["complex"]
    print(f"{name}: {nw} weights, m={cfg.m}, L={len(cfg.q_bits)}"
          f"{', encrypted denominator' if enc_denom else ''}")
    for p, c in cases.items():
        print(f"  {p:8s} B={c.B:4d} cts  {c.bytes / 1e6:9.2f} MB per client"
              f"  max err vs w/8 {c.err:.2e}")
    for phase in r.phases:
        a, b = r.ms[phase], x.ms[phase]
        ma, mb = statistics.median(a), statistics.median(b)
        clear = max(b) < min(a)
        print(f"  {phase:24s} real {ma:8.3f} [{min(a):8.3f} .. {max(a):8.3f}]"
              f"  complex {mb:8.3f} [{min(b):8.3f} .. {max(b):8.3f}]"
              f"  x{ma / mb:5.2f}"
              f"  {'beyond the spread' if clear else 'WITHIN the spread'}")
    del cases, r, x
    torch.cuda.empty_cache()
