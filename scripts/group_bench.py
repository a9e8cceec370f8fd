"""Model groups against the only thing the single-model engine offers: G handles stepped one after the other.

    python scripts/group_bench.py [--out profiles/group_sup_bench.json] [--groups 1 2 4 6 8 16] [--blocks 9] [--steps 100]

The reference's baseline size (D = 1200, batch 20, mr_nn.py), inputs resident on the device, fp32 and bf16.  For every
(dtype, G): one group handle of G models (G = 1: a single handle on both sides, the spread of the method) and G single
handles in one process; blocks of `steps` supervised steps alternate between the two sides, each block timed by a host clock
around work that ends in a device synchronise, each under a time limit of its own; the figure is the median over the blocks
of a side, in ms per step of ALL G models (the sequential side: G single steps).  With --profile-g G a second, separate pass
takes the per-kernel profile (mrgan_profile_begin / _end) of one grouped and one single step at that G.

    python scripts/group_bench.py --gan [--out profiles/group_gan_bench.json] [--groups 2 4 6 8 16] [--profile-g 6]

--gan: the same method applied to the GAN hot loop at the reference's size (D = 1200, batch 50, N = 6000 rows resident, stream
mode, graph replay): one group handle stepped through train_pair_group against G single handles stepped one after the other
through train_pair; a step is one (D, G) pair of ALL G models.

Every (dtype, G) runs in a child process of its own under a time limit; the first failure ends the run."""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, B = 1200, 20
BLOCK_LIMIT_S = 60          # per timed block (100 steps of 16 models take well under a second)


class BlockTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise BlockTimeout("a timed block ran into its time limit")


def worker(dtype, G, blocks, steps, profile):
    import numpy as np
    import torch
    from mr_gan_amd import engine as E
    from mr_gan_amd.mr_nn import NN_BETA_1, NN_LR
    from mr_gan_amd.model import glorot_uniform
    dev = "cuda:0"
    rng = np.random.RandomState(1)

    def make(models, seed):
        cfg = E.default_config(D, B)
        cfg.dtype = E.BF16 if dtype == 'bf16' else E.F32
        cfg.lr, cfg.beta1, cfg.seed, cfg.models = NN_LR, NN_BETA_1, seed, models
        eng = E.Engine(cfg, dev)
        for m in range(max(1, models)):
            r = np.random.RandomState(seed + m)
            ws = []
            for i in range(eng.num_tensors(E.NET_D)):
                shp = eng.full_shape(E.NET_D, i)
                ws.append(glorot_uniform(r, shp[0], shp[1]) if len(shp) == 2 else np.zeros(shp, np.float32))
            if models > 1:
                eng.select_model(m)
            eng.set_weights(E.NET_D, ws)
        return eng

    x = torch.from_numpy(rng.standard_normal((G, B, D)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.randint(0, 6, (G, B)).astype(np.int32)).to(dev)
    singles = [make(0, 100 + m) for m in range(G)]
    sargs = [E.Engine.sup_args(x[m], y[m]) for m in range(G)]
    if G > 1:
        group, gargs = make(G, 100), E.Engine.sup_group_args(x, y)

    def seq_block(n):
        for _ in range(n):
            for eng, a in zip(singles, sargs):
                eng.sup_step(a, want_outputs=False)

    def grp_block(n):
        if G == 1:
            return seq_block(n)
        for _ in range(n):
            group.sup_step_group(gargs, want_outputs=False)

    signal.signal(signal.SIGALRM, _alarm)

    def timed(fn):
        signal.alarm(BLOCK_LIMIT_S)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        signal.alarm(0)
        return (t1 - t0) * 1e3 / steps

    for fn in (seq_block, grp_block):           # warm up both sides: code objects, caches, clocks
        fn(30)
    torch.cuda.synchronize()
    seq, grp = [], []
    for _ in range(blocks):
        seq.append(timed(seq_block))
        grp.append(timed(grp_block))
    res = dict(dtype=dtype, G=G, steps_per_block=steps, blocks=blocks, seq_ms=seq, grp_ms=grp,
               seq_median_ms=float(np.median(seq)), grp_median_ms=float(np.median(grp)))
    res['speedup'] = res['seq_median_ms'] / res['grp_median_ms']
    res['spread_pct'] = dict(seq=100.0 * (max(seq) - min(seq)) / res['seq_median_ms'], grp=100.0 * (max(grp) - min(grp)) / res['grp_median_ms'])
    if profile and G > 1:
        # per-kernel device times of one step on each side (event pairs around every launch: a pass of its own)
        def prof(eng, step):
            step()
            torch.cuda.synchronize()
            eng.profile_begin()
            for _ in range(10):
                step()
            return {k: dict(us=1e2 * v[0], launches=v[1] // 10) for k, v in eng.profile_end().items()}
        res['profile_group_us_per_step'] = prof(group, lambda: group.sup_step_group(gargs, want_outputs=False))
        res['profile_single_us_per_step'] = prof(singles[0], lambda: singles[0].sup_step(sargs[0], want_outputs=False))
    for e in singles + ([group] if G > 1 else []):
        e.close()
    print("RESULT " + json.dumps(res))


GAN_B, GAN_N = 50, 6000      # mr_gan.py's batch; a fold's training rows


def gan_worker(dtype, G, blocks, steps, profile):
    import numpy as np
    import torch
    from mr_gan_amd import engine as E
    from mr_gan_amd.model import init_weights
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    if steps > GAN_N // GAN_B:
        raise SystemExit("--steps: a block is at most one epoch of the index streams (%d batches)" % (GAN_N // GAN_B))

    def make(models, seed):
        cfg = E.default_config(D, GAN_B)
        cfg.dtype = E.BF16 if dtype == 'bf16' else E.F32
        cfg.seed, cfg.models, cfg.flags = seed, models, E.FLAG_GRAPH
        eng = E.Engine(cfg, dev)
        for m in range(max(1, models)):          # Keras' default initialisation from a seed, through the selected model
            eng.select_model(m)
            init_weights(eng, (E.NET_G, E.NET_D), seed + m)
        eng.select_model(0)
        return eng

    stream = torch.cuda.Stream(dev)      # (graph capture is not permitted on the legacy default stream)
    with torch.cuda.stream(stream):
        t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
        X = t(rng.standard_normal((GAN_N, D)).astype(np.float32))
        XL = t(rng.standard_normal((600, D)).astype(np.float32))
        idx_lab = rng.randint(0, 600, (G, GAN_N)).astype(np.int32)
        lab = t(rng.randint(0, 6, 600).astype(np.int32)[idx_lab], torch.int32)
        idx_lab = t(idx_lab, torch.int32)
        idx_u1 = t(np.stack([rng.permutation(GAN_N) for _ in range(G)]), torch.int32)
        idx_u2 = t(np.stack([rng.permutation(GAN_N) for _ in range(G)]), torch.int32)
        singles = [make(0, 100 + m) for m in range(G)]
        sargs = [(E.Engine.disc_args(XL, lab[m], X, None, idx_lab[m], idx_u1[m], stream_mode=1),
                  E.Engine.gen_args(X, None, idx_u2[m], stream_mode=1)) for m in range(G)]
        group = make(G, 100)
        gd = E.Engine.disc_group_args(XL, lab, X, None, idx_lab, idx_u1, stream_mode=1)
        gg = E.Engine.gen_group_args(X, None, idx_u2, stream_mode=1)

        def seq_block(n):
            for eng in singles:
                eng.set_iterations(0, 0)          # (rewinds the batch counter of the index streams)
            for _ in range(n):
                for eng, (da, ga) in zip(singles, sargs):
                    eng.train_pair(da, ga)

        def grp_block(n):
            group.set_iterations(0, 0)
            for _ in range(n):
                group.train_pair_group(gd, gg)

        signal.signal(signal.SIGALRM, _alarm)

        def timed(fn):
            signal.alarm(BLOCK_LIMIT_S)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(steps)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            signal.alarm(0)
            return (t1 - t0) * 1e3 / steps

        for fn in (seq_block, grp_block):           # warm up both sides: code objects, graph capture, caches, clocks
            fn(30)
        torch.cuda.synchronize()
        seq, grp = [], []
        for _ in range(blocks):
            seq.append(timed(seq_block))
            grp.append(timed(grp_block))
        res = dict(dtype=dtype, G=G, steps_per_block=steps, blocks=blocks, seq_ms=seq, grp_ms=grp,
                   seq_median_ms=float(np.median(seq)), grp_median_ms=float(np.median(grp)))
        res['speedup'] = res['seq_median_ms'] / res['grp_median_ms']
        res['spread_pct'] = dict(seq=100.0 * (max(seq) - min(seq)) / res['seq_median_ms'], grp=100.0 * (max(grp) - min(grp)) / res['grp_median_ms'])
        if profile:
            def prof(eng, step):
                eng.set_iterations(0, 0)
                step()
                torch.cuda.synchronize()
                eng.profile_begin()
                for _ in range(10):
                    step()
                return {k: dict(us=1e2 * v[0], launches=v[1] // 10) for k, v in eng.profile_end().items()}
            res['profile_group_us_per_pair'] = prof(group, lambda: group.train_pair_group(gd, gg))
            res['profile_single_us_per_pair'] = prof(singles[0], lambda: singles[0].train_pair(*sargs[0]))
        for e in singles + [group]:
            e.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gan', action='store_true', help='the GAN hot loop (train_pair_group against G x train_pair) instead of the supervised step')
    ap.add_argument('--out', default=None)
    ap.add_argument('--groups', type=int, nargs='+', default=None)
    ap.add_argument('--dtypes', nargs='+', default=['float32', 'bf16'])
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--profile-g', type=int, nargs='*', default=[])
    ap.add_argument('--worker', nargs=2, metavar=('DTYPE', 'G'))
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'group_gan_bench.json' if args.gan else 'group_sup_bench.json')
    if args.groups is None:
        args.groups = [2, 4, 6, 8, 16] if args.gan else [1, 2, 4, 6, 8, 16]
    if args.gan and min(args.groups) < 2:
        ap.error("--gan: a group has at least 2 models")
    if args.blocks < 5:
        ap.error("--blocks: the median needs at least 5 blocks per side")
    if args.worker:
        return (gan_worker if args.gan else worker)(args.worker[0], int(args.worker[1]), args.blocks, args.steps, int(args.worker[1]) in args.profile_g)
    results = []
    for dtype in args.dtypes:
        for G in args.groups:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', dtype, str(G), '--blocks', str(args.blocks), '--steps', str(args.steps)]
            cmd += (['--gan'] if args.gan else []) + ['--profile-g'] + [str(g) for g in args.profile_g]
            try:
                out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=240, check=True).stdout.decode()
            except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as e:
                print("group_bench: %s G=%d failed (%s); stopping here" % (dtype, G, e), file=sys.stderr)
                break
            line = [l for l in out.splitlines() if l.startswith("RESULT ")][-1]
            r = json.loads(line[len("RESULT "):])
            results.append(r)
            print("%-8s G=%-2d  sequential %.4f ms  grouped %.4f ms  per G-step   x%.2f   (block spread %.1f %% / %.1f %%)"
                  % (dtype, G, r['seq_median_ms'], r['grp_median_ms'], r['speedup'], r['spread_pct']['seq'], r['spread_pct']['grp']), flush=True)
        else:
            continue
        break
    shape = dict(D=D, batch=GAN_B, rows=GAN_N, step="one (D, G) pair of all G models, stream mode, graph replay") if args.gan else dict(D=D, batch=B)
    doc = dict(command="python scripts/group_bench.py " + " ".join(sys.argv[1:]), shape=shape, results=results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if len(results) == len(args.dtypes) * len(args.groups) else 1


if __name__ == '__main__':
    sys.exit(main())
