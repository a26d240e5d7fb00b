"""Time the graph-replayed denoise step per prediction objective at the config-4
base shape (unet1, 1x3x16x64x64, bf16 autocast), DDPM and DDIM eta = 0:
eps, x0, v, and v with dynamic thresholding, interleaved in one session.

  python tools/objective_step_ab.py [--out profiles/objective_step_ab.txt] [--repeats 5]
                                    [--parent-pkg DIR]

--parent-pkg names a built `dalle2-video_amd` directory of the parent commit.
Its eps step is then measured first, by this same script in a child process
(`--pkg DIR --eps-only`), so both trees are timed on the same box in one run.

The per-step time is differential, as in tools/ddim_step_ab.py: two loops of A
and B steps, (t_B - t_A) / (B - A); the spread is max - min of the repeats.
The library calls of one eager step are counted as well (every ops entry point
goes through `ops.call`): an objective must add none, dynamic thresholding
adds the quantile kernel."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 16, 80
SHAPE = dict(frame_sizes=(64,), frame_numbers=(16,))
OBJECTIVES = {"eps": {}, "x0": dict(predict_x_start=True), "v": dict(predict_v=True),
              "v+dyn": dict(predict_v=True, use_dynamic_thres=True)}
SAMPLERS = {"ddpm": lambda n: dict(timesteps=n),
            "ddim_eta0": lambda n: dict(timesteps=1000, sample_timesteps=n, ddim_sampling_eta=0.0)}


def measure(pkg, eps_only, repeats):
    sys.path.insert(0, pkg)
    import torch
    from dalle2_video import ops
    from dalle2_video.dalle2_video import Unet3D, VideoDecoder
    from dalle2_video.utils import deterministic_fill_

    def decoder(unet, **kw):
        d = VideoDecoder(unet=(unet,), learned_variance=False, **SHAPE, **kw)
        if unet is None or not getattr(unet, "_filled", False):
            deterministic_fill_(d.unets[0])
            d.unets[0]._filled = True
        else:
            d.unets[0] = unet  # VideoDecoder rebuilds the unet it is given: share the filled one
        return d

    def loop_s(dec, emb):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vid = dec.sample(video_embed=emb, one_unet_in_gpu_at_time=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        assert torch.isfinite(vid).all(), "non-finite sample"
        return dt

    def eager_calls(dec, emb):
        """library calls of one eager denoise step (differential over two loop lengths)"""
        counts = []
        real = ops.call
        for d in dec:
            n = [0]

            def counting(*a, **kw):
                n[0] += 1
                return real(*a, **kw)

            ops.call, d.sample_graphs = counting, False
            try:
                loop_s(d, emb)
            finally:
                ops.call, d.sample_graphs = real, True
            counts.append(n[0])
        return (counts[1] - counts[0]) / (B - A)

    first = decoder(Unet3D(64, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8)), timesteps=A)
    u = first.unets[0]
    names = ["eps"] if eps_only else list(OBJECTIVES)
    variants = {}
    for sname, skw in SAMPLERS.items():
        for oname in names:
            variants[f"{sname} {oname}"] = tuple(decoder(u, **skw(n), **OBJECTIVES[oname]).to("cuda") for n in (A, B))
    emb = torch.randn(1, 512, device="cuda")
    for pair in variants.values():  # warm-up: every lazily allocated workspace exists
        loop_s(pair[0], emb)
    steps = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (da, db) in variants.items():
            ta, tb = loop_s(da, emb), loop_s(db, emb)
            steps[k].append(1e3 * (tb - ta) / (B - A))
    calls = {k: eager_calls(pair, emb) for k, pair in variants.items()}
    return {"device": torch.cuda.get_device_name(0), "steps_ms": steps, "calls": calls}


def rows(tag, res):
    out = []
    for k, ms in res["steps_ms"].items():
        out.append(f"{tag:7s} {k:16s} {statistics.median(ms):9.4f} {min(ms):8.4f} {max(ms):8.4f} "
                   f"{max(ms) - min(ms):9.4f} {res['calls'][k]:10.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None, help="built dalle2-video_amd directory of the parent commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dalle2-video_amd"))
    ap.add_argument("--eps-only", action="store_true")
    ap.add_argument("--json", action="store_true", help="print the raw result as one JSON line")
    args = ap.parse_args()
    if args.json:
        print("RESULT " + json.dumps(measure(args.pkg, args.eps_only, args.repeats)), flush=True)
        return
    parent = None
    if args.parent_pkg:  # a fresh child process, before this one opens the GPU
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", args.parent_pkg, "--eps-only",
                              "--json", "--repeats", str(args.repeats)], check=True, capture_output=True,
                             text=True).stdout
        parent = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = measure(args.pkg, args.eps_only, args.repeats)
    lines = [f"graph-replayed denoise step, unet1 1x3x16x64x64 bf16, {res['device']}",
             f"differential over loops of {A} and {B} steps, {args.repeats} interleaved repeats;",
             "calls/step: library calls of one eager step",
             "tree    variant          median ms   min ms   max ms spread ms calls/step"]
    if parent:
        lines += rows("parent", parent)
    lines += rows("this", res)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
