"""Time of one mrgan_input_gradient call next to mrgan_predict_logits of the same rows on the same handle: wall time per call
(hipEvents around `reps` calls on one stream, after a warm-up) and one profiled call each (mrgan_profile_begin /
mrgan_profile_end) for the per-kernel split.

    python scripts/saliency_bench.py [--d 1200 --rows 1200 --batches 50 4096 --dtype bf16 --reps 20]
    python scripts/saliency_bench.py --method smoothgrad --draws 16      (or --method integrated)
With --method the line also carries one mrgan_attribution call of `draws` draws (smoothgrad: the network's own sigmas;
integrated: zero baseline, times the input) beside `draws` plain calls timed in the same run, and its per-kernel split.
Prints one JSON line per batch size."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mr_gan_amd import engine as E  # noqa: E402
from mr_gan_amd.model import MRGAN  # noqa: E402


def timed(fn, reps, stream):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def profiled(eng, fn):
    eng.profile_begin()
    fn()
    return {k: dict(ms=round(v[0], 4), launches=v[1]) for k, v in sorted(eng.profile_end().items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=1200)
    ap.add_argument("--rows", type=int, default=1200)
    ap.add_argument("--batches", type=int, nargs="+", default=[50, 4096])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--method", default=None, choices=["smoothgrad", "integrated"])
    ap.add_argument("--draws", type=int, default=16)
    args = ap.parse_args()
    rs = np.random.RandomState(3)
    X = rs.randn(args.rows, args.d).astype(np.float32)
    for batch in args.batches:
        m = MRGAN(args.d, batch_size=batch, dtype='bfloat16' if args.dtype == 'bf16' else 'float32', seed=77, use_graph=False)
        eng = m.engine
        with m._on_stream():
            x = m._dev(X)
            out = torch.empty((args.rows, args.d), dtype=torch.float32, device=m.device)
            cls = torch.empty((args.rows,), dtype=torch.int32, device=m.device)
            res = dict(d=args.d, rows=args.rows, batch=batch, dtype=args.dtype)
            for name, post in (("raw", E.SAL_RAW), ("heatmap", E.SAL_HEATMAP)):
                call = lambda post=post: eng.input_gradient(x, None, E.SAL_XENT, post, out=out, classes_out=cls)
                res["input_gradient_%s_ms" % name] = round(timed(call, args.reps, m.stream), 4)
            res["predict_logits_ms"] = round(timed(lambda: eng.predict_logits(x), args.reps, m.stream), 4)
            res["input_gradient_kernels"] = profiled(eng, lambda: eng.input_gradient(x, None, E.SAL_XENT, E.SAL_HEATMAP, out=out, classes_out=cls))
            res["predict_logits_kernels"] = profiled(eng, lambda: eng.predict_logits(x))
            if args.method:
                kw = dict(E.attribution_plan(args.method, args.draws, own_sigmas=(float(eng.cfg.sigma[0]), float(eng.cfg.sigma[1]))))
                attr = lambda: eng.attribution(x, None, E.SAL_XENT, E.SAL_HEATMAP, out=out, classes_out=cls, **kw)
                plain = lambda: eng.input_gradient(x, None, E.SAL_XENT, E.SAL_HEATMAP, out=out, classes_out=cls)
                reps = max(2, args.reps // 4)
                res.update(method=args.method, draws=args.draws)
                res["attribution_ms"] = round(timed(attr, reps, m.stream), 4)
                res["plain_calls_ms"] = round(timed(lambda: [plain() for _ in range(args.draws)], reps, m.stream), 4)      # draws x the plain call
                res["attribution_kernels"] = profiled(eng, attr)
        eng.close()
        print(json.dumps(res))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
