"""Hoisted multi-step rotations and the encrypted linear transform on one GPU
at the config #2 and config #5 rings, full weight-vector ciphertext counts
(the shapes of scripts/bench_rotate.py), top level and one below:

  rotations   rotate_many_tensor over G exact-key steps  vs  the loop of G
              rotate_tensor calls (what the tree offered before)
  transform   LinearTransform.apply_tensor with G diagonals  vs  the same sum
              composed of rotate_tensor + mul_plain + add, plaintexts encoded
              beforehand on both sides

for G in {2, 8, 32}. The two paths are warmed, then alternated, and timed with
a host clock around iterations that end in a device synchronise; median
[min..max] over the samples. Their outputs differ in the low bits by design
(tests/test_hoist_cpu.py), so they are not compared here. Results are dropped
as they are produced so that the loop holds one rotation at a time. At the
config #5 ring rotate_many_tensor is called on chunks of CHUNK steps (each
chunk decomposes again): [32, 683, 2, 5, 2^15] int64 and its mod-down
intermediates do not fit comfortably. Each ring runs in a child process of
its own under a time limit; a child that fails or overruns ends the run.

  python scripts/bench_hoist.py            # both rings
  python scripts/bench_hoist.py m13        # one ring, in this process
"""
import sys, os, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import subprocess

# name -> (m, chain, weights, iterations per sample, G chunk, child limit [s])
RINGS = {"m13": (8192, (60, 40), 222_722, 20, 32, 300),
         "m15": (32768, (60, 40, 40, 40), 11_181_642, 2, 8, 600)}
GS = (2, 8, 32)
SAMPLES = 5


def run(name):
    import numpy as np
    import torch
    from hefl.config import HEConfig
    from hefl.he import LinearTransform
    from hefl.he.ckks import CKKSContext, Ciphertext, CtxtTensor, Plaintext

    m, chain, nw, iters, chunk, _ = RINGS[name]
    ctx = CKKSContext(HEConfig(m=m, scale_bits=40, q_bits=chain, seed=1),
                      device="cuda")
    kp = ctx.keygen()
    steps_all = list(range(1, max(GS) + 1))
    gk = ctx.galois_keygen(kp.sk, steps=steps_all)
    B = (nw + ctx.slots - 1) // ctx.slots
    rng = np.random.default_rng(3)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    def compare(label, new, old):
        new(); old()                               # warm-up of both paths
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(SAMPLES):
            ms[0].append(timed(new))
            ms[1].append(timed(old))
        a, b = sorted(ms[0]), sorted(ms[1])
        print(f"{label}: new {np.median(a):.3f} ms [{a[0]:.3f}..{a[-1]:.3f}] | "
              f"old {np.median(b):.3f} ms [{b[0]:.3f}..{b[-1]:.3f}] | "
              f"new/old {np.median(a) / np.median(b):.3f}", flush=True)

    for l in (ctx.L, ctx.L - 1):
        # uniform residues: the cost does not depend on the plaintext
        data = torch.stack([torch.randint(0, q, (B, 2, ctx.n), device="cuda",
                                          dtype=torch.int64)
                            for q in ctx.primes[:l]], dim=-2)
        ct = CtxtTensor(data, ctx.scale, nw)
        head = (f"{name} m={m} chain={chain} level={l} B={B} "
                f"({data.numel() * 8 / 2**20:.0f} MiB)")
        for G in GS:
            steps = steps_all[:G]

            def hoisted():
                for s in range(0, G, chunk):
                    outs = ctx.rotate_many_tensor(ct, steps[s:s + chunk], gk)
                    del outs

            def loop():
                for s in steps:
                    out = ctx.rotate_tensor(ct, s, gk)
                    del out

            compare(f"{head} rotations G={G} chunk={min(chunk, G)}",
                    hoisted, loop)

            diags = {k: rng.uniform(-1, 1, ctx.slots) for k in steps}
            lt = LinearTransform.from_diagonals(ctx, diags, level=l)
            pts = [Plaintext(lt.pt[b], lt.scale) for b in range(G)]

            def transform():
                out = lt.apply_tensor(ct, gk)
                del out

            def composed():
                acc = None
                for k, pt in zip(steps, pts):
                    term = ctx.mul_plain(
                        Ciphertext(ctx.rotate_data(ct.data, k, gk), ct.scale), pt)
                    acc = term if acc is None else ctx.add(acc, term)
                del acc

            compare(f"{head} transform G={G}", transform, composed)
            del lt, pts
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
