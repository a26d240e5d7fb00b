"""Cost of inpainting in the graph-replayed DDIM step at the config-4 base
shape (unet1, 1x3x16x64x64, bf16 autocast), and the blend kernel on its own.

  python tools/inpaint_step_ab.py [--out profiles/inpaint_step_ab.txt] [--repeats 5]

Step rate: as tools/ddim_step_ab.py measures it, differential over loops of A
and B DDIM steps ((t_B - t_A) / (B - A): the two eager steps, the capture and
the fresh weight-image cache cancel), plain and with inpainting at
inpaint_resample_times=1 (one noise draw and one dv_inpaint_blend more per
step, and one blend after the loop), interleaved in one session.  The spread is
max - min of the repeats.

Kernel: ops.TIMER brackets every dv_inpaint_blend launch with events; the
three variants (blend, blend + renoise, final) at the clip shape, where the
launch is all there is to see, at 4x3x16x256x256 (x, known and noise together
151 MB: they stay in the 256 MiB last-level cache from launch to launch, so
this is not an HBM rate) and at 8x3x16x256x256 (302 MB: past that cache).
Bytes are what the call moves: x, known (and noise) read, x written, the mask
once.  The kernel skips 4-pixel groups it has nothing to write to, so blend
and final run on an all-known mask, where every element is read and written;
blend + renoise touches every element under any mask (half the frames known)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle2-video_amd"))
import torch  # noqa: E402

from dalle2_video import ops  # noqa: E402
from dalle2_video.dalle2_video import Unet3D, VideoDecoder  # noqa: E402
from dalle2_video.utils import deterministic_fill_  # noqa: E402

A, B = 16, 80
FRAMES, SIZE = 16, 64


def decoder(unet, steps, fill=False):
    d = VideoDecoder(unet=(unet,), learned_variance=False, frame_sizes=(SIZE,), frame_numbers=(FRAMES,),
                     timesteps=1000, sample_timesteps=steps, ddim_sampling_eta=0.0)
    if fill:
        deterministic_fill_(d.unets[0])
    else:
        d.unets[0] = unet  # VideoDecoder rebuilds the unet it is given: share the filled one
    return d


def loop_s(dec, emb, inpaint):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = dec.sample(video_embed=emb, one_unet_in_gpu_at_time=False, **inpaint)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert torch.isfinite(vid).all(), "non-finite sample"
    return dt


def kernel_lines(sched, shape, reps):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).cuda()
    known = torch.rand(shape, generator=g).cuda()
    noise = torch.randn(shape, generator=g).cuda()
    mask = torch.zeros(shape[0], *shape[2:], dtype=torch.uint8, device="cuda")
    mask[:, : shape[2] // 2] = 1  # the first half of the frames is known
    t = torch.full((shape[0],), 537, dtype=torch.long, device="cuda")
    u = torch.full((shape[0],), 500, dtype=torch.long, device="cuda")
    full = torch.ones_like(mask)
    variants = {"blend": dict(mask=full, noise=noise, times=t),
                "blend+renoise": dict(mask=mask, noise=noise, times=t, times_from=u),
                "final": dict(mask=full, noise=None, times=None, final=True)}
    lines = []
    for name, kw in variants.items():
        run = lambda: ops.inpaint_blend(x, known, kw["mask"], kw.get("noise"), kw.get("times"), sched,
                                        times_from=kw.get("times_from"), normalize=True, final=kw.get("final", False))
        for _ in range(5):
            run()
        ops.TIMER = ops.KernelTimer()
        try:
            for _ in range(reps):
                run()
            s = ops.TIMER.summary()["inpaint_blend_kernel"]
        finally:
            ops.TIMER = None
        us = 1e3 * s["ms"] / s["count"]
        nbytes = s["bytes"] / s["count"]
        lines.append(f"{'x'.join(map(str, shape)):18s} {name:14s} {us:9.2f} {nbytes / 1e6:10.2f} "
                     f"{nbytes / (us * 1e-6) / 1e12:8.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda"
    first = decoder(Unet3D(64, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8)), A, fill=True)
    u = first.unets[0]
    pair = (first.to(dev), decoder(u, B).to(dev))
    emb = torch.randn(1, 512, device=dev)
    g = torch.Generator().manual_seed(1)
    video = torch.rand(1, 3, FRAMES, SIZE, SIZE, generator=g).to(dev)
    mask = torch.zeros(1, FRAMES, SIZE, SIZE, dtype=torch.bool, device=dev)
    mask[:, : FRAMES // 2] = True
    variants = {"plain": {}, "inpaint_r1": dict(inpaint_video=video, inpaint_mask=mask, inpaint_resample_times=1)}
    for kw in variants.values():  # warm-up: every lazily allocated workspace exists
        loop_s(pair[0], emb, kw)
    steps = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, kw in variants.items():
            ta, tb = loop_s(pair[0], emb, kw), loop_s(pair[1], emb, kw)
            steps[k].append((tb - ta) / (B - A))
    lines = [f"graph-replayed DDIM step (eta 0), unet1 1x3x{FRAMES}x{SIZE}x{SIZE} bf16, {torch.cuda.get_device_name(0)}",
             f"differential over loops of {A} and {B} steps, {args.repeats} interleaved repeats",
             "variant      median ms   min ms   max ms   spread ms   steps/s (median)"]
    for k, v in steps.items():
        ms = [1e3 * s for s in v]
        med = statistics.median(ms)
        lines.append(f"{k:12s} {med:9.4f} {min(ms):8.4f} {max(ms):8.4f} {max(ms) - min(ms):11.4f} {1e3 / med:12.1f}")
    lines.append("dv_inpaint_blend alone (ops.TIMER event brackets, mean of 50 launches after 5 warm-up launches)")
    lines.append("shape              variant          us/call   MB moved     TB/s")
    sched = pair[0].noise_schedulers[0]
    for shape in ((1, 3, FRAMES, SIZE, SIZE), (4, 3, 16, 256, 256), (8, 3, 16, 256, 256)):
        lines += kernel_lines(sched, shape, 50)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
