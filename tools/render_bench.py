"""Cost of ps_render: ms per render of all envs through the closeup camera, rgb only and all three
outputs (rgb, depth and segmentation: three calls, as BatchedPianoEnv.render returns one image kind
per call), at 84 x 84 and 240 x 320, beside one bare step on the same handle. States: 50
random-action steps of the benchmark's song (Crossing Field) on the default hull hand. Medians of 7,
timed with HIP events. Also the mean length of the tiles' culled object lists (of the 153 records).
usage: python tools/render_bench.py [--envs 4096] [--reps 7] [--out FILE]"""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def event_ms(torch, fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    dp = importlib.import_module("diffusion-piano_amd")
    R = dp.rendering
    n = args.envs
    seq = dp.music.parse_midi(ROOT / "tests" / "data" / "Crossing Field Cut 10s.mid")
    env = dp.BatchedPianoEnv(n, seq, dp.TaskConfig(trim_silence=True, primitive_fingertip_collisions=False),
                             device="cuda:0", seed=12345)
    gen = torch.Generator(device="cuda:0").manual_seed(12345)
    actions = [torch.rand(n, env.action_dim, device="cuda:0", generator=gen) * 2 - 1 for _ in range(16)]
    env.reset()
    for t in range(50):
        env.step(actions[t % 16])
    torch.cuda.synchronize()
    lines = [f"# tools/render_bench.py: {n} envs, closeup camera, hull hand, Crossing Field after 50 random-action steps;",
             f"# ms per call of all {n} envs, median of {args.reps} (HIP events) [min .. max]"]
    snap = env.snapshot()

    def step():
        env.step(actions[0])

    step()  # (warm)
    ms = []
    for _ in range(args.reps):  # every timed step starts from the same states
        env.restore(snap)
        ms += event_ms(torch, step, 1)
    env.restore(snap)
    lines.append(f"step                      {np.median(ms):8.3f} ms [{min(ms):.3f} .. {max(ms):.3f}]")
    for h, w in ((84, 84), (240, 320)):
        kinds = {"rgb": lambda: env.render("closeup", h, w),
                 "rgb + depth + seg": lambda: (env.render("closeup", h, w), env.render("closeup", h, w, depth=True),
                                               env.render("closeup", h, w, segmentation=True))}
        for name, fn in kinds.items():
            fn()  # (warm: the first call allocates)
            torch.cuda.synchronize()
            ms = event_ms(torch, fn, args.reps)
            pix = n * h * w * (3 if "+" in name else 1)
            lines.append(f"{h:3d} x {w:3d} {name:17s} {np.median(ms):8.3f} ms [{min(ms):.3f} .. {max(ms):.3f}]  "
                         f"{pix / np.median(ms) / 1e6:.2f} Gpixel/s")
        R.list_stats(env)
        R.render(env, "closeup", h, w, count_list=True)
        total, tiles = R.list_stats(env)
        lines.append(f"{h:3d} x {w:3d} tile list: mean {total / tiles:.2f} of 153 objects over {tiles} tiles")
    env.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
