"""ms per mrgan_ae_step (one train_on_batch(x, x) of the autoencoder pre-stage) at the reference's shape -- D 9600 (0.2 s of the
contact microphone), encoder nodes 1024 / 512 / 256, batch 32 (others/mr_gan_autoencoder.py) -- and at batch 4096, in fp32 and
bf16, with the per-kernel times of one profiled pass (mrgan_profile_begin / mrgan_profile_end); and, as the outside yardstick,
the same MLP's Adam step in eager PyTorch on the same card (fp32, and under bfloat16 autocast with fp32 master weights).

Both sides gather their batch from a resident fp32 matrix through an index vector.  The engine and the eager model alternate in
blocks inside one process; a block is sized to last about --block-seconds, every shape is warmed up first, the host clock runs
around work that ends in a device synchronise.

    python scripts/autoencoder_bench.py [--d 9600 --nodes 1024 512 256 --batches 32 4096] [--blocks 5 --block-seconds 0.5]
Prints one JSON line per (batch, dtype)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mr_gan_amd import engine as E  # noqa: E402
from mr_gan_amd.autoencoder import AE_BETA_1, AE_LR, encoder_widths  # noqa: E402


def glorot(rs, shape):
    lim = np.sqrt(6.0 / sum(shape))
    return rs.uniform(-lim, lim, size=shape).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=9600)
    ap.add_argument("--nodes", type=int, nargs=3, default=[1024, 512, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 4096])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--profile-steps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autoencoder_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D, widths = args.d, encoder_widths(args.nodes)
    dims = (D,) + widths + (D,)
    rs = np.random.RandomState(3)
    for B in args.batches:
        rows = max(2 * B, 4096)
        X = torch.from_numpy(rs.randn(rows, D).astype(np.float32)).to(dev)
        weights = []
        for l in range(6):
            weights += [glorot(rs, (dims[l], dims[l + 1])), np.zeros(dims[l + 1], np.float32)]
        for dtype in args.dtypes:
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                print(json.dumps(measure(args, dev, X, B, dtype, widths, weights)))
                sys.stdout.flush()


def measure(args, dev, X, B, dtype, widths, weights):
    D, rows = X.shape[1], X.shape[0]
    max_steps = 4000
    idx = torch.randint(0, rows, ((max_steps + 1) * B,), dtype=torch.int32, device=dev)
    # ---- the engine ----
    cfg = E.default_config(D, B)
    cfg.dtype, cfg.seed, cfg.flags = {"bf16": E.BF16, "f32": E.F32}[dtype], 1, E.FLAG_AUTOENCODER
    cfg.lr, cfg.beta1, cfg.sigma = AE_LR, AE_BETA_1, (C.c_float * 5)()
    for i, w in enumerate(widths):
        cfg.d_hidden[i] = w
    eng = E.Engine(cfg, dev)
    eng.set_weights(E.NET_D, weights)
    args_stream = E.Engine.ae_args(X, idx, stream_mode=1)
    done = [0]

    def run_engine(n):
        eng.set_iterations(done[0], 0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            eng.ae_step(args_stream, want_outputs=False)
        torch.cuda.synchronize(dev)
        done[0] += n
        return time.perf_counter() - t0

    # ---- eager PyTorch: the same MLP, mse, Adam at Keras' defaults ----
    layers = []
    for l in range(6):
        lin = torch.nn.Linear(weights[2 * l].shape[0], weights[2 * l].shape[1], device=dev)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(weights[2 * l].T))
            lin.bias.zero_()
        layers += [lin] + ([torch.nn.ReLU()] if l < 5 else [])
    mlp = torch.nn.Sequential(*layers)
    opt = torch.optim.Adam(mlp.parameters(), lr=AE_LR, betas=(AE_BETA_1, 0.999), eps=1e-8)
    idx64 = idx.long()
    pos = [0]

    def run_torch(n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            x = X.index_select(0, idx64[pos[0] * B:(pos[0] + 1) * B])
            pos[0] = (pos[0] + 1) % max_steps
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
                loss = torch.nn.functional.mse_loss(mlp(x).float(), x)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    sides = dict(engine=run_engine, torch_eager=run_torch)
    steps, ms = {}, {k: [] for k in sides}
    for name, run in sides.items():                         # warm up, then size a block to about block_seconds
        run(args.warmup)
        per = run(args.warmup) / args.warmup
        steps[name] = int(min(max_steps // (args.blocks + 2), max(args.warmup, args.block_seconds / per)))
    for _ in range(args.blocks):                            # engine / eager / engine / eager ...
        for name, run in sides.items():
            ms[name].append(1e3 * run(steps[name]) / steps[name])
    # ---- one profiled pass of the engine: us per step of every kernel ----
    eng.set_iterations(done[0], 0)
    eng.profile_begin()
    for _ in range(args.profile_steps):
        eng.ae_step(args_stream, want_outputs=False)
    prof = eng.profile_end()
    kern = {k: dict(us=round(1e3 * v[0] / args.profile_steps, 2), launches=v[1] // args.profile_steps) for k, v in prof.items()}
    loss = eng.ae_step(args_stream)
    eng.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return dict(d=D, nodes=list(widths[:3]), batch=B, dtype=dtype, blocks=args.blocks, steps_per_block=steps,
                engine_ms_per_step=[round(v, 4) for v in ms["engine"]], engine_median_ms=round(med["engine"], 4),
                torch_eager_ms_per_step=[round(v, 4) for v in ms["torch_eager"]], torch_eager_median_ms=round(med["torch_eager"], 4),
                engine_over_torch=round(med["engine"] / med["torch_eager"], 3),
                kernel_us_per_step=kern, kernel_sum_us=round(sum(v["us"] for v in kern.values()), 1),
                dominant_kernel=max(kern, key=lambda k: kern[k]["us"]), engine_loss_after=round(loss, 5))


if __name__ == "__main__":
    main()
