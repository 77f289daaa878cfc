"""Throughput of the one-hand task: the benchmark's workload (Crossing
Field, random canonical actions, staggered episodes, bench.py's warmup and step counts) with one
hand only, timed on two legs that step the SAME detached-hand model:

  one   ps_task_cfg.hand_side set: the one-hand task;
  two   ps_task_cfg.hand_side = 0: the two-hand task, to which that model is one with locked dofs.

Both legs run the same step kernels and differ in the task layer; above 2048 envs `two` is
time-sliced and `one` is not (csrc/pianosim.hip launch()).

Every repetition times both legs one after the other (interleaved), each from a fresh reset.
usage: python tools/one_hand_bench.py [--envs 4096 1024] [--hands hull capsule] [--reps 3]
       [--steps 50] [--warmup 5] [--out FILE]"""
import argparse
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HANDS = {"hull": dict(primitive_fingertip_collisions=False), "capsule": {}}


def timed(env, actions, steps, warmup, torch):
    """env-steps/s of `steps` steps after `warmup` untimed ones, from a fresh staggered reset."""
    env.reset()
    T = env.song.T
    env.set_state({"t_idx": (np.arange(env.num_envs) % T).astype(np.int32)})
    for i in range(warmup):
        env.step(actions[i % len(actions)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        env.step(actions[(warmup + i) % len(actions)])
    torch.cuda.synchronize()
    return env.num_envs * steps / (time.perf_counter() - t0)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, nargs="+", default=[4096, 1024])
    p.add_argument("--hands", nargs="+", default=["hull", "capsule"], choices=list(HANDS))
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--side", default="right", choices=["right", "left"])
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    dp = importlib.import_module("diffusion-piano_amd")
    seq = dp.music.parse_midi(ROOT / "tests" / "data" / "Crossing Field Cut 10s.mid")
    lines = [f"# tools/one_hand_bench.py: Crossing Field, {args.side} hand, random canonical actions, "
             f"{args.warmup} warmup + {args.steps} timed steps, {args.reps} interleaved repetitions; env-steps/s",
             "# one = hand_side set (the one-hand task); two = the same model, hand_side 0 (the two-hand task); same step kernels; one is never time-sliced, two is above 2048 envs"]
    for n in args.envs:
        for hand in args.hands:
            md, st, tc = dp.compile_task(seq, dp.TaskConfig(trim_silence=True, hand_side=args.side, **HANDS[hand]))
            tc0 = dp.abi.TaskCfg.from_buffer_copy(tc)
            tc0.hand_side = dp.abi.HAND_BOTH
            legs = {"one": dp.BatchedPianoEnv.from_compiled(n, md, st, tc, device="cuda:0", seed=12345),
                    "two": dp.BatchedPianoEnv.from_compiled(n, md, st, tc0, device="cuda:0", seed=12345)}
            gen = torch.Generator(device="cuda:0").manual_seed(12345)
            pool = max(1, min(args.steps + args.warmup, 64))
            actions = [torch.rand(n, legs["one"].action_dim, device="cuda:0", generator=gen) * 2 - 1 for _ in range(pool)]
            res = {k: [] for k in legs}
            for _ in range(args.reps):
                for k, env in legs.items():
                    res[k].append(timed(env, actions, args.steps, args.warmup, torch))
            for env in legs.values():
                env.close()
            one, two = res["one"], res["two"]
            lines.append(f"envs {n:5d} hand {hand:8s} one " + " ".join(f"{v:10.0f}" for v in one) +
                         "   two " + " ".join(f"{v:10.0f}" for v in two) +
                         f"   one min/two max {min(one) / max(two):.3f}  medians {np.median(one) / np.median(two):.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
