"""Cost of the extra observables (TaskConfig.observables): the benchmark's
workload (Crossing Field, random canonical actions, staggered episodes, bench.py's warmup and step
counts) on three handles that differ in the row they write:

  none        the default row (319 wide);
  joints_vel  the default row + both hands' joints_vel (+52);
  all         every extra observable (+501).

Every repetition times the three legs one after the other (interleaved), each from a fresh reset.
usage: python tools/observables_bench.py [--envs 4096] [--hands hull capsule] [--reps 3]
       [--steps 50] [--warmup 5] [--out FILE]"""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from one_hand_bench import HANDS, timed  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, nargs="+", default=[4096])
    p.add_argument("--hands", nargs="+", default=["hull", "capsule"], choices=list(HANDS))
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    dp = importlib.import_module("diffusion-piano_amd")
    seq = dp.music.parse_midi(ROOT / "tests" / "data" / "Crossing Field Cut 10s.mid")
    sets = {"none": None, "joints_vel": ["joints_vel"], "all": list(dp.abi.OBSERVABLES)}
    lines = [f"# tools/observables_bench.py: Crossing Field, random canonical actions, {args.warmup} warmup + "
             f"{args.steps} timed steps, {args.reps} interleaved repetitions; env-steps/s",
             "# none = the default row; joints_vel = + both hands' joints_vel; all = every extra observable"]
    for n in args.envs:
        for hand in args.hands:
            legs = {k: dp.BatchedPianoEnv(n, seq, dp.TaskConfig(trim_silence=True, observables=obs, **HANDS[hand]),
                                          device="cuda:0", seed=12345) for k, obs in sets.items()}
            gen = torch.Generator(device="cuda:0").manual_seed(12345)
            pool = max(1, min(args.steps + args.warmup, 64))
            actions = [torch.rand(n, legs["none"].action_dim, device="cuda:0", generator=gen) * 2 - 1 for _ in range(pool)]
            res = {k: [] for k in legs}
            for _ in range(args.reps):
                for k, env in legs.items():
                    res[k].append(timed(env, actions, args.steps, args.warmup, torch))
            widths = {k: env.obs_dim for k, env in legs.items()}
            for env in legs.values():
                env.close()
            base = np.median(res["none"])
            lines.append(f"envs {n:5d} hand {hand:8s} " + "   ".join(
                f"{k} (row {widths[k]}) " + " ".join(f"{v:9.0f}" for v in res[k]) + f" median/none {np.median(res[k]) / base:.3f}"
                for k in legs))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
