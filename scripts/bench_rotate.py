"""rotate_tensor cost on one GPU at the config #2 and config #5 rings, full
weight-vector ciphertext counts: the fused path (galois_lift + galois_perm_add)
against the path composed of torch.index_select / torch.where /
bcast_center_mod / modadd_limbs / torch.stack around the same key-switch
(HEFL_GALOIS_FUSED=0). The two are alternated, timed with a host clock around
iterations that end in a device synchronise, and checked bit-identical at the
timed size. Each ring runs in a child process of its own under a time limit;
a child that fails or overruns ends the run.

  python scripts/bench_rotate.py            # both rings
  python scripts/bench_rotate.py m13        # one ring, in this process
"""
import sys, os, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import subprocess

# name -> (m, chain, weights, iterations per sample, child time limit [s])
RINGS = {"m13": (8192, (60, 40), 222_722, 200, 240),
         "m15": (32768, (60, 40, 40, 40), 11_181_642, 10, 420)}
SAMPLES = 5


def run(name):
    import numpy as np
    import torch
    from hefl.config import HEConfig
    from hefl.he.ckks import CKKSContext, CtxtTensor

    m, chain, nw, iters, _ = RINGS[name]
    ctx = CKKSContext(HEConfig(m=m, scale_bits=40, q_bits=chain, seed=1),
                      device="cuda")
    kp = ctx.keygen()
    gk = ctx.galois_keygen(kp.sk, steps=[1])
    B = (nw + ctx.slots - 1) // ctx.slots

    def sample(fused):
        os.environ["HEFL_GALOIS_FUSED"] = "1" if fused else "0"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = ctx.rotate_tensor(ct, 1, gk)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3, out

    for l in (ctx.L, ctx.L - 1):
        # uniform residues: rotation cost does not depend on the plaintext
        data = torch.stack([torch.randint(0, q, (B, 2, ctx.n), device="cuda",
                                          dtype=torch.int64)
                            for q in ctx.primes[:l]], dim=-2)
        ct = CtxtTensor(data, ctx.scale, nw)
        _, a = sample(True)
        _, b = sample(False)                       # warm-up of both paths
        same = torch.equal(a.data, b.data)
        del a, b
        ms = {True: [], False: []}
        for _ in range(SAMPLES):
            for fused in (True, False):
                ms[fused].append(sample(fused)[0])
        f, c = (sorted(ms[k]) for k in (True, False))
        print(f"{name} m={m} chain={chain} level={l} B={B} "
              f"({data.numel() * 8 / 2**20:.0f} MiB): "
              f"fused {np.median(f):.3f} ms [{f[0]:.3f}..{f[-1]:.3f}] | "
              f"composed {np.median(c):.3f} ms [{c[0]:.3f}..{c[-1]:.3f}] | "
              f"fused/composed {np.median(f) / np.median(c):.3f} | "
              f"bit-identical {same}", flush=True)
        if not same:
            sys.exit(1)
        del data, ct


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for name, ring in RINGS.items():
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), name],
                                timeout=ring[-1]).returncode
            if rc != 0:
                sys.exit(f"{name}: exit {rc}")
