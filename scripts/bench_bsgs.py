"""Baby-step/giant-step LinearTransform on one GPU at the config #2 ring
(n = 2^13, chain (60, 40)), top level and one below:

  crossover   apply_tensor with bsgs="auto"  vs  the diagonal method, for
              G in {32, 256} diagonals (steps 0 .. G-1) on R = 28 ciphertexts
  dense       the 4096 x 4096 transform (4096 diagonals), which only BSGS can
              hold: time at R = 1 and R = 28, key bytes, plaintext bytes, and
              the host-side encoding time of its diagonals
  bsgs_mac    the multiply-accumulate kernel alone on the dense transform's
              operands, against the bytes the algorithm needs (every plaintext
              and baby word read once, every u word written once; with more
              babies than one LDS tile u is read and written once more per
              further tile, which is counted too)

The paths are warmed, then alternated, and timed with a host clock around
iterations that end in a device synchronise; median [min..max] over the
samples. Ciphertexts and Galois keys are uniform residues of the right shapes
(the cost depends on neither, and hundreds of real keys would only add key
generation time); the diagonals are encoded for real. The ring runs in a child process
under a time limit; a child that fails or overruns ends the run.

  python scripts/bench_bsgs.py            # the ring, in a child process
  python scripts/bench_bsgs.py m13        # in this process
"""
import sys, os, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import subprocess

# name -> (m, chain, ciphertexts, iterations per sample, child limit [s])
RINGS = {"m13": (8192, (60, 40), 28, 5, 540)}
GS = (32, 256)
SAMPLES = 5
MIB = float(2 ** 20)


def run(name, device="cuda"):
    import numpy as np
    import torch
    from hefl.config import HEConfig
    from hefl.he import LinearTransform
    from hefl.he.ckks import CKKSContext, CtxtTensor

    m, chain, R_full, iters, _ = RINGS[name]
    ctx = CKKSContext(HEConfig(m=m, scale_bits=40, q_bits=chain, seed=1),
                      device=device)
    sync = torch.cuda.synchronize
    n, slots, L = ctx.n, ctx.slots, ctx.L
    rng = np.random.default_rng(3)
    all_primes = ctx.primes[:L] + [ctx.special]

    def residues(lead, primes):
        return torch.stack([torch.randint(0, q, tuple(lead) + (n,),
                                          device=device, dtype=torch.int64)
                            for q in primes], dim=-2)

    gk = {}

    def keys_for(steps):
        for s in steps:
            g = ctx.galois_element(s)
            if g not in gk:
                gk[g] = residues((L, 2), all_primes)      # [L, 2, L+1, n]
        return gk

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        sync()
        return (time.perf_counter() - t0) / iters * 1e3

    def sample(fns):
        for fn in fns:
            fn()                                   # warm-up of every path
        sync()
        ms = [[] for _ in fns]
        for _ in range(SAMPLES):
            for out, fn in zip(ms, fns):
                out.append(timed(fn))
        return [sorted(v) for v in ms]

    def fmt(v):
        return f"{np.median(v):.3f} ms [{v[0]:.3f}..{v[-1]:.3f}]"

    def applier(lt, ct):
        def fn():
            out = lt.apply_tensor(ct, gk)
            del out
        return fn

    for l in (L, L - 1):
        if l < 1:
            continue
        head = f"{name} n={m} chain={chain} level={l}"
        key_mib = l * 2 * (l + 1) * n * 8 / MIB    # one key's slice at level l
        ct = CtxtTensor(residues((R_full, 2), ctx.primes[:l]), ctx.scale,
                        R_full * slots)
        for G in GS:
            diags = {k: rng.uniform(-1, 1, slots) for k in range(G)}
            lt_d = LinearTransform.from_diagonals(ctx, diags, level=l)
            lt_b = LinearTransform.from_diagonals(ctx, diags, level=l,
                                                  bsgs="auto")
            keys_for(lt_d.steps + lt_b.steps)
            b, d = sample([applier(lt_b, ct), applier(lt_d, ct)])
            print(f"{head} R={R_full} G={G}: bsgs n1={lt_b.n1} "
                  f"({len(lt_b.steps)} keys) {fmt(b)} | diagonal "
                  f"({len(lt_d.steps)} keys) {fmt(d)} | bsgs/diagonal "
                  f"{np.median(b) / np.median(d):.3f}", flush=True)
            del lt_d, lt_b
            ctx.__dict__.pop("_galois_stack_cache", None)
        gk.clear()

        t0 = time.perf_counter()
        M = rng.uniform(-1, 1, (slots, slots))
        lt = LinearTransform(ctx, M, level=l, bsgs="auto")
        sync()
        enc_s = time.perf_counter() - t0
        del M
        keys_for(lt.steps)
        print(f"{head} dense {slots}x{slots}: n1={lt.n1}, {len(lt.steps)} keys "
              f"= {len(lt.steps) * key_mib:.1f} MiB at this level "
              f"({len(lt.steps) * L * 2 * (L + 1) * n * 8 / MIB:.1f} MiB as "
              f"generated), plaintexts {lt.pt.numel() * 8 / MIB:.0f} MiB, "
              f"set-up (diagonals, host encode, NTT) {enc_s:.1f} s", flush=True)
        for R in (1, R_full):
            sub = CtxtTensor(ct.data[:R].contiguous(), ctx.scale, R * slots)
            (t,) = sample([applier(lt, sub)])
            print(f"{head} dense R={R}: apply_tensor {fmt(t)}, peak allocated "
                  f"{torch.cuda.max_memory_allocated() / MIB:.0f} MiB",
                  flush=True)
            be = ctx.backend
            rot = residues((len(lt.baby_elements), R, 2), ctx.primes[:l])

            def mac():
                u = be.bsgs_mac(sub.data, rot, lt.pt, lt.goff, lt.bidx, lt.has0)
                del u
            (t,) = sample([mac])
            Nb, Ng = len(lt.baby_steps), len(lt.giant_steps)
            tiles = -(-Nb // be._C.BSGS_BABY_TILE)
            u_bytes = Ng * R * 2 * l * n * 8
            nbytes = (lt.pt.numel() * 8 + Nb * R * 2 * l * n * 8
                      + u_bytes * (2 * tiles - 1))
            print(f"{head} dense R={R}: bsgs_mac {fmt(t)}, "
                  f"{nbytes / MIB:.0f} MiB needed -> "
                  f"{nbytes / (np.median(t) * 1e-3) / 1e9:.0f} GB/s", flush=True)
            del rot, sub
        del lt, ct
        gk.clear()
        ctx.__dict__.pop("_galois_stack_cache", None)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        run(sys.argv[1])
    else:
        for name, ring in RINGS.items():
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), name],
                                timeout=ring[-1]).returncode
            if rc != 0:
                sys.exit(f"{name}: exit {rc}")
