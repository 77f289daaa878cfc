"""What the predictive-sampling planner costs and what it plays (planning.PredictiveSampler).

1. Timing, on the benchmark's song and hand (bench.py's defaults): one ``act()`` at G = 1,
   C = 4096, H = 8 - a snapshot save, two restores, perturb, H x (action, step, accumulate),
   select and the real step - against H + 1 bare ``env.step`` calls on the same handle. The
   difference is the planner's own overhead.
2. One Twinkle episode played by the planner's leader, and by uniformly random actions, with each
   one's ``musical_metrics`` (precision, recall, F1 of the episode).

    python tools/plan_bench.py [--out profiles/plan_bench.txt]
"""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(torch, fn, reps):
    """median wall time of fn() in ms over reps, the device drained before and after each"""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=str(ROOT / "profiles" / "plan_bench.txt"))
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--horizon", type=int, default=8)
    p.add_argument("--knots", type=int, default=4)
    p.add_argument("--sigma", type=float, default=0.2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--play-envs", type=int, default=1024, help="candidates of the Twinkle episode's planner")
    args = p.parse_args(argv)
    import torch
    import bench
    dp = importlib.import_module("diffusion-piano_amd")
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    N, H, P = args.envs, args.horizon, args.knots

    # -- 1. act() against H + 1 bare steps
    seq, task = bench.load_song(dp, "crossing_field")
    task.primitive_fingertip_collisions = bench.HANDS["hull"][0]
    env = dp.BatchedPianoEnv(N, seq, task, device="cuda:0")
    env.reset()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    rand = lambda: torch.rand(N, env.action_dim, device="cuda:0", generator=gen) * 2 - 1
    acts = [rand() for _ in range(H + 1)]
    for a in acts:
        env.step(a)
    ps = dp.PredictiveSampler(env, groups=1, horizon=H, knots=P, sigma=args.sigma, interpolation="linear")

    def bare():
        for a in acts:
            env.step(a)

    def dry():  # the planner's own launches of one plan(): everything but the H env steps
        step = env.step
        env.step = lambda a: None
        try:
            ps.plan()
        finally:
            env.step = step

    ps.act(), bare(), dry()  # warm-up
    t_act1, _ = timed(torch, ps.act, args.reps)
    t_bare1, _ = timed(torch, bare, args.reps)
    t_dry1, _ = timed(torch, dry, args.reps)
    t_act2, _ = timed(torch, ps.act, args.reps)
    t_bare2, _ = timed(torch, bare, args.reps)
    t_dry2, _ = timed(torch, dry, args.reps)
    t_bare, t_dry = min(t_bare1, t_bare2), min(t_dry1, t_dry2)
    say(f"plan_bench: crossing_field, hull hand, G=1 C={N} H={H} P={P} linear; medians of {args.reps}, two rounds")
    say(f"  act()                        {t_act1:8.3f} ms {t_act2:8.3f} ms")
    say(f"  {H + 1} bare env.step (random)    {t_bare1:8.3f} ms {t_bare2:8.3f} ms")
    say(f"  plan() without its env steps {t_dry1:8.3f} ms {t_dry2:8.3f} ms   (save, 2 restores, perturb, "
        f"{H} x (action, accumulate), select; snapshot {ps._snap.bytes / 2 ** 20:.1f} MiB)")
    say(f"  the planner's own launches are {100 * t_dry / t_bare:.1f}% of the bare steps. act() itself is not the "
        f"bare steps plus that: its {H} rollout steps start from {N} copies of one state and cost what those "
        f"states cost, the bare steps what {N} different states under random actions cost.")
    ps.close(), env.close()

    # -- 2. one Twinkle episode: the planner's leader, and random actions
    tw = dp.music.twinkle_twinkle_little_star_one_hand()
    C = args.play_envs
    env = dp.BatchedPianoEnv(C, tw, dp.TaskConfig(), device="cuda:0")
    env.reset()
    ps = dp.PredictiveSampler(env, groups=1, horizon=H, knots=P, sigma=args.sigma, interpolation="linear")
    total, steps = 0.0, 0
    for steps in range(1, 100000):
        _, r, _, st = ps.act()
        total += float(r[0])
        if int(st[0]) == dp.abi.LAST:
            break
    ep, cnt = env.musical_metrics()
    m = ep[0].cpu().numpy()
    say(f"twinkle, planner (C={C} H={H} P={P} sigma={args.sigma}): {steps} steps, return {total:.2f}, "
        f"precision {m[0]:.3f} recall {m[1]:.3f} F1 {m[2]:.3f} (episodes {int(cnt[0])})")
    ps.close(), env.close()
    env = dp.BatchedPianoEnv(64, tw, dp.TaskConfig(), device="cuda:0")
    env.reset()
    total = torch.zeros(64, device="cuda:0")
    for steps in range(1, 100000):
        _, r, _, st = env.step(torch.rand(64, env.action_dim, device="cuda:0", generator=gen) * 2 - 1)
        total += r
        if int(st[0]) == dp.abi.LAST:
            break
    m = env.musical_metrics()[0].cpu().numpy().mean(axis=0)
    say(f"twinkle, random actions (mean of 64 envs): {steps} steps, return {float(total.mean()):.2f}, "
        f"precision {m[0]:.3f} recall {m[1]:.3f} F1 {m[2]:.3f}")
    env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
