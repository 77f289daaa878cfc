"""Cost of the per-episode MIDI augmentations on bench.py's workload (development aid; bench.py
is the contract): N Crossing Field envs, hull hand, episodes staggered so ~N/T envs restart every
step. Three configurations:

  plain     a plain handle
  prob0     the same handle with every variation at prob 0: the songs and T are those of the
            plain handle, only the builder launch and the per-env tables add cost
  augment   [MidiTemporalStretch(1.0, 0.1), MidiPitchShift(1.0, 2)]

usage: python tools/augment_bench.py [--envs N] [--steps K] [--warmup W] [--blocks B]
                                     [--config plain prob0 augment] [--out FILE]
Prints one JSON line per configuration (env-steps/s: the median of B timed blocks of K steps).
The builder kernel's own time: run one configuration under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
dp = importlib.import_module("diffusion-piano_amd")
V = dp.variations


def configs():
    return {"plain": None,
            "prob0": [V.MidiTemporalStretch(0.0, 0.1), V.MidiPitchShift(0.0, 2)],
            "augment": [V.MidiTemporalStretch(1.0, 0.1), V.MidiPitchShift(1.0, 2)]}


def run(name, augs, n, steps, warmup, blocks):
    seq = dp.music.parse_midi(ROOT / "tests" / "data" / "Crossing Field Cut 10s.mid")
    task = dp.TaskConfig(trim_silence=True, primitive_fingertip_collisions=False, augmentations=augs)
    env = dp.BatchedPianoEnv(n, seq, task, device="cuda:0", seed=12345)
    env.reset()
    T = env.augmentation()["T"].cpu().numpy() if augs is not None else np.full(n, env.song.T)
    env.set_state({"t_idx": (np.arange(n) % T).astype(np.int32)})  # bench.py stagger_episodes
    gen = torch.Generator(device="cuda:0").manual_seed(12345)
    actions = [torch.rand(n, env.action_dim, device="cuda:0", generator=gen) * 2 - 1 for _ in range(64)]
    for i in range(warmup):
        env.step(actions[i % 64])
    rates = []
    for b in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            env.step(actions[(warmup + b * steps + i) % 64])
        torch.cuda.synchronize()
        rates.append(n * steps / (time.perf_counter() - t0))
    rec = {"config": name, "envs": n, "steps": steps, "blocks": blocks,
           "env_steps_per_s": float(np.median(rates)), "min": float(min(rates)), "max": float(max(rates))}
    if augs is not None:
        a = env.augmentation()
        rec.update(T_cap=env.T_cap, table_bytes=n * env.T_cap * dp.abi.AUG_ROW_BYTES,
                   T_min=int(a["T"].min()), T_max=int(a["T"].max()), fallbacks=int(a["fallbacks"].sum()))
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--config", nargs="+", default=list(configs()))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for name in args.config:
        rec = run(name, configs()[name], args.envs, args.steps, args.warmup, args.blocks)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
