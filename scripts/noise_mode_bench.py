"""ms per (D, G) pair with the default Irwin-Hall generator and with noise='gaussian' (MRGAN_FLAG_GAUSS_NOISE), timed the way
bench.py times the flagship workload: train_pair through graph replay, inputs resident in HBM, index streams, device-drawn z.
The two handles alternate in blocks on one device inside one process; then one profiled pass per mode (mrgan_profile_begin /
mrgan_profile_end) for the per-kernel time of the noisy forward variants and stage_kernel.

    python scripts/noise_mode_bench.py [--d 512 --batch 4096 --dtype bf16] [--steps 200 --blocks 5]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mr_gan_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32", "fp8"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, D = args.batch, args.d
    rs = np.random.RandomState(3)
    rows = max(8 * B, 4096)
    X = torch.from_numpy(rs.randn(rows, D).astype(np.float32)).to(dev)
    n_rows = (max(args.steps, args.warmup, args.profile_steps) + 4) * B
    idx = [torch.from_numpy(rs.randint(0, rows, size=n_rows).astype(np.int32)).to(dev) for _ in range(3)]
    labels = torch.from_numpy(rs.randint(0, 6, size=n_rows).astype(np.int32)).to(dev)
    stream = torch.cuda.Stream(dev)
    modes = {}
    with torch.cuda.stream(stream):
        for name in E.NOISE_MODES:
            cfg = E.default_config(D, B)
            cfg.dtype = {"bf16": E.BF16, "f32": E.F32, "fp8": E.FP8}[args.dtype]
            cfg.seed = 1
            cfg.flags = E.FLAG_GRAPH | E.noise_flags(name)
            eng = E.Engine(cfg, dev)
            ws = np.random.RandomState(7)
            for net in (E.NET_G, E.NET_D):
                w = []
                for i in range(eng.num_tensors(net)):
                    shp = eng.full_shape(net, i)
                    lim = np.sqrt(6.0 / sum(shp)) if len(shp) == 2 else 0.0
                    w.append(ws.uniform(-lim, lim, size=shp).astype(np.float32) if len(shp) == 2
                             else (np.ones(shp, np.float32) if (net == E.NET_G and i == 2) else np.zeros(shp, np.float32)))
                eng.set_weights(net, w)
            dargs = E.Engine.disc_args(X, labels, X, None, idx[0], idx[1], stream_mode=1)
            gargs = E.Engine.gen_args(X, None, idx[2], stream_mode=1)
            modes[name] = dict(eng=eng, dargs=dargs, gargs=gargs, done=0, ms=[])

        def run(m, n):
            m["eng"].set_iterations(2 * m["done"], 0)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                m["eng"].train_pair(m["dargs"], m["gargs"])
            torch.cuda.synchronize(dev)
            m["done"] += n
            return time.perf_counter() - t0

        for m in modes.values():
            run(m, args.warmup)
        for _ in range(args.blocks):                        # off / on / off / on ...
            for m in modes.values():
                m["ms"].append(1e3 * run(m, args.steps) / args.steps)
        out = dict(d=D, batch=B, dtype=args.dtype, steps=args.steps, blocks=args.blocks)
        for name, m in modes.items():
            m["eng"].set_iterations(2 * m["done"], 0)
            m["eng"].profile_begin()
            for _ in range(args.profile_steps):
                m["eng"].train_pair(m["dargs"], m["gargs"])
            prof = m["eng"].profile_end()
            # us per step of the kernels that draw noise: stage_kernel, the chain's forward launches, forward GEMM variants
            kern = {k: round(1e3 * v[0] / args.profile_steps, 2) for k, v in prof.items()
                    if k.startswith(("stage_kernel", "chain_kernel<0", "chain_kernel<1", "gemm_bf16_kc_kernel<0", "gemm_f32_kernel<0", "gemm_fp8_kc_kernel<0"))}
            out[name] = dict(ms_per_step=[round(v, 4) for v in m["ms"]], median_ms=round(float(np.median(m["ms"])), 4), kernel_us_per_step=kern)
            m["eng"].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
