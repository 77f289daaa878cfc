"""Plays the recorded Twinkle action trace (tests/data/twinkle_twinkle_actions.npy, canonical
actions) on one env and writes what it looks and sounds like: a PNG per control step and the
episode's .mid (the env's own MIDI recorder) into a directory.
usage: python tools/render_episode.py OUT_DIR [--camera closeup] [--height 240] [--width 320] [--steps N]"""
import argparse
import importlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("--camera", default="closeup")
    p.add_argument("--height", type=int, default=240)
    p.add_argument("--width", type=int, default=320)
    p.add_argument("--steps", type=int, default=None, help="control steps (default: the whole episode)")
    args = p.parse_args(argv)
    import torch

    dp = importlib.import_module("diffusion-piano_amd")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    env = dp.BatchedPianoEnv(1, dp.music.twinkle_twinkle_little_star_one_hand(), dp.TaskConfig(), device="cuda:0")
    env.record_midi()
    trace = np.load(ROOT / "tests" / "data" / "twinkle_twinkle_actions.npy").astype(np.float32)
    env.reset()
    kw = dict(camera=args.camera, height=args.height, width=args.width, change_color_on_activation=True)
    dp.write_png(out / "step_0000.png", env.render(**kw)[0])
    steps = min(args.steps or env.song.T, env.song.T)
    for t in range(steps):
        _, _, _, st = env.step(torch.from_numpy(trace[t % len(trace)][None, :env.action_dim]).to("cuda:0"))
        dp.write_png(out / f"step_{t + 1:04d}.png", env.render(**kw)[0])
        if int(st[0]) == dp.StepType.LAST:
            break
    # (the recorder swaps its banks at the next reset, not at LAST: the episode is still the running one)
    dp.music.write_midi(env.performance(0, "current"), out / "episode.mid")
    print(f"{t + 2} images and episode.mid in {out}")
    env.close()


if __name__ == "__main__":
    main()
