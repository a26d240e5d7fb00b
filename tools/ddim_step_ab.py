"""Time the graph-replayed denoise step of the three samplers at the config-4
base shape (unet1, 1x3x16x64x64, bf16 autocast): DDPM, DDIM eta = 0, DDIM
eta = 1, interleaved in one session.

  python tools/ddim_step_ab.py [--out profiles/ddim_step_ab.txt] [--repeats 5]

The per-step time is differential, as bench.py's sampling legs measure it: two
loops of A and B steps, (t_B - t_A) / (B - A), so the per-loop constant (two
eager steps, the capture, a fresh weight-image cache) cancels.  The spread is
max - min of the repeats.  Also times whole loops: 50 DDIM steps and 1000 DDPM
steps of a 1000-step schedule."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle2-video_amd"))
import torch  # noqa: E402

from dalle2_video.dalle2_video import Unet3D, VideoDecoder  # noqa: E402
from dalle2_video.utils import deterministic_fill_  # noqa: E402

A, B = 16, 80
SHAPE = dict(frame_sizes=(64,), frame_numbers=(16,))


def decoder(unet, fill=False, **kw):
    d = VideoDecoder(unet=(unet,), learned_variance=False, **SHAPE, **kw)
    if fill:
        deterministic_fill_(d.unets[0])
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda"
    first = decoder(Unet3D(64, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8)), fill=True, timesteps=A)
    u = first.unets[0]
    variants = {
        "ddpm": (first, decoder(u, timesteps=B)),
        "ddim_eta0": tuple(decoder(u, timesteps=1000, sample_timesteps=s, ddim_sampling_eta=0.0) for s in (A, B)),
        "ddim_eta1": tuple(decoder(u, timesteps=1000, sample_timesteps=s, ddim_sampling_eta=1.0) for s in (A, B)),
    }
    for pair in variants.values():
        for d in pair:
            d.to(dev)
    emb = torch.randn(1, 512, device=dev)
    for pair in variants.values():  # warm-up: every lazily allocated workspace exists
        loop_s(pair[0], emb)
    steps = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (da, db) in variants.items():
            ta, tb = loop_s(da, emb), loop_s(db, emb)
            steps[k].append((tb - ta) / (B - A))
    lines = [f"graph-replayed denoise step, unet1 1x3x16x64x64 bf16, {torch.cuda.get_device_name(0)}",
             f"differential over loops of {A} and {B} steps, {args.repeats} interleaved repeats",
             "variant      median ms   min ms   max ms   spread ms"]
    for k, v in steps.items():
        ms = [1e3 * s for s in v]
        lines.append(f"{k:12s} {statistics.median(ms):9.4f} {min(ms):8.4f} {max(ms):8.4f} {max(ms) - min(ms):11.4f}")
    full = {"ddim 50 of 1000 (eta 0)": decoder(u, timesteps=1000, sample_timesteps=50, ddim_sampling_eta=0.0),
            "ddim 50 of 1000 (eta 1)": decoder(u, timesteps=1000, sample_timesteps=50, ddim_sampling_eta=1.0),
            "ddpm 1000": decoder(u, timesteps=1000)}
    lines.append("whole sample() loop, second call (seconds):")
    for k, d in full.items():
        d.to(dev)
        loop_s(d, emb)
        lines.append(f"{k:24s} {loop_s(d, emb):8.3f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
