"""Cost of video-embedding conditioning (Unet3D(cond_on_video_embeds=True): 7-key
cross attention, two more small linears, the mask selects) at the config-4 base
shape (unet1, 1x3x16x64x64, bf16 autocast), next to the unconditioned unet:

  sampling   the graph-replayed DDIM eta = 0 denoise step, differential over two
             loop lengths as in tools/objective_step_ab.py: (t_B - t_A) / (B - A)
  training   one eager forward + backward of decoder(video, video_embed), timed
             with device events after warm-up
  launches   library calls of one eager denoise step / one training pass (every
             ops entry point goes through `ops.call`)

  python tools/video_cond_ab.py [--out profiles/video_cond_ab.txt] [--repeats 5]
                                [--parent-pkg DIR]

--parent-pkg names a built `dalle2-video_amd` directory of the parent commit.
Its unconditioned numbers are then measured first, by this same script in a
child process (`--pkg DIR --uncond-only`), so both trees are timed on the same
box in one run.  The spread is max - min of the repeats."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 8, 40
SHAPE = dict(frame_sizes=(64,), frame_numbers=(16,))


def measure(pkg, uncond_only, repeats):
    sys.path.insert(0, pkg)
    import torch
    from dalle2_video import ops
    from dalle2_video.dalle2_video import Unet3D, VideoDecoder
    from dalle2_video.utils import deterministic_fill_

    emb = torch.randn(1, 512, device="cuda")
    video = torch.rand(1, 3, 16, 64, 64, device="cuda")

    def unet(cond):
        kw = dict(cond_on_video_embeds=True) if cond else {}
        return Unet3D(64, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8), **kw)

    def decoder(u, n):
        d = VideoDecoder(unet=(u,), learned_variance=False, timesteps=1000, sample_timesteps=n,
                         ddim_sampling_eta=0.0, **SHAPE)
        if not getattr(d.unets[0], "_filled", False):
            deterministic_fill_(d.unets[0])
            with torch.no_grad():  # the fill zeroes to_out: give the step something to carry
                d.unets[0].to_out.weight.normal_(0, 0.05)
            d.unets[0]._filled = True
        return d.cuda()

    def counted(fn):
        n, real = [0], ops.call

        def counting(*a, **kw):
            n[0] += 1
            return real(*a, **kw)

        ops.call = counting
        try:
            fn()
        finally:
            ops.call = real
        return n[0]

    def loop_s(dec):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vid = dec.sample(video_embed=emb, one_unet_in_gpu_at_time=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        assert torch.isfinite(vid).all(), "non-finite sample"
        return dt

    def train_pass(dec):
        for p in dec.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = dec(video, video_embed=emb, unet_number=1)
        loss.backward()
        return loss

    out = {}
    for name in ("uncond",) if uncond_only else ("uncond", "cond"):
        u = unet(name == "cond")
        da = decoder(u, A)
        db = decoder(da.unets[0], B)
        db.unets[0] = da.unets[0]
        res = {}
        # launches of one eager denoise step
        cnt = []
        for d in (da, db):
            d.sample_graphs = False
            cnt.append(counted(lambda: loop_s(d)))
            d.sample_graphs = True
        res["step_calls"] = (cnt[1] - cnt[0]) / (B - A)
        for d in (da, db):  # warm-up: capture
            loop_s(d)
        steps = []
        for _ in range(repeats):
            ta, tb = loop_s(da), loop_s(db)
            steps.append((tb - ta) / (B - A) * 1e3)
        res["step_ms"] = statistics.median(steps)
        res["step_spread_ms"] = max(steps) - min(steps)
        da.train()
        torch.cuda.manual_seed(0)
        for _ in range(3):
            train_pass(da)
        res["train_calls"] = counted(lambda: train_pass(da))
        times = []
        for _ in range(repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            train_pass(da)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times = times[2:]
        res["train_ms"] = statistics.median(times)
        res["train_spread_ms"] = max(times) - min(times)
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dalle2-video_amd"))
    ap.add_argument("--uncond-only", action="store_true")
    a = ap.parse_args()
    if a.uncond_only:
        print("RESULT " + json.dumps(measure(a.pkg, True, a.repeats)))
        return
    rows = {}
    if a.parent_pkg:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", a.parent_pkg, "--uncond-only",
                            "--repeats", str(a.repeats)], capture_output=True, text=True, check=True, timeout=900)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        rows["parent uncond"] = json.loads(line[7:])["uncond"]
    here = measure(a.pkg, False, a.repeats)
    rows["this uncond"], rows["this cond"] = here["uncond"], here["cond"]
    lines = ["video-embedding conditioning A/B, unet1 1x3x16x64x64 bf16 autocast, one MI355X, one session",
             f"sampling: graph-replayed DDIM eta=0 step, differential over {A}/{B}-step loops; training: eager "
             f"forward+backward; median of {a.repeats}, spread = max - min",
             f"{'':16s}{'step ms':>10s}{'spread':>9s}{'calls':>8s}{'train ms':>10s}{'spread':>9s}{'calls':>8s}"]
    for k, r in rows.items():
        lines.append(f"{k:16s}{r['step_ms']:10.3f}{r['step_spread_ms']:9.3f}{r['step_calls']:8.1f}"
                     f"{r['train_ms']:10.3f}{r['train_spread_ms']:9.3f}{r['train_calls']:8d}")
    c, u = rows["this cond"], rows["this uncond"]
    lines.append(f"conditioning adds {c['step_ms'] - u['step_ms']:+.3f} ms and {c['step_calls'] - u['step_calls']:+.1f} "
                 f"calls per sampling step, {c['train_ms'] - u['train_ms']:+.3f} ms and "
                 f"{c['train_calls'] - u['train_calls']:+d} calls per training pass")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
