"""The time-sliced step's queue, observed: who ran which (env, chunk) item when, from the
-DPS_QTRACE build (diffusion-piano_amd/libpianosim_qtrace.so; csrc/kernel_v2.inc QT_*). Every
item run leaves the 100 MHz clock at three points - its workgroup turns to the queue, the chunk
begins, the chunk ends - with the ticket it was popped at (none: the workgroup's first item, or
a continuation it ran itself) and the workgroup; every workgroup leaves its exit time and the
tickets it took that held no item. bench.py's workload (episodes staggered, uniform random
actions), STEPS traced steps after WARM untraced ones; the tables are means over the steps.

Envs are grouped by rank decile of order_kernel's order of the step (decile 0: the envs
expected longest; the last one holds the envs due for their auto-reset, one short chunk).

usage: python tools/queue_trace.py [N] [hull|primitive|authored|both] [song]"""
import ctypes as C
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
os.environ.setdefault("PIANOSIM_LIB", str(ROOT / "diffusion-piano_amd" / "libpianosim_qtrace.so"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
dp = importlib.import_module("diffusion-piano_amd")
lib = importlib.import_module("diffusion-piano_amd._lib")
from helpers import song, tool_hand_kwargs  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
HAND = sys.argv[2] if len(sys.argv) > 2 else "both"
NAME = sys.argv[3] if len(sys.argv) > 3 else "crossing_field"
WARM, STEPS, DEC = 5, 10, 10
US = 0.01  # microseconds per tick of the 100 MHz clock


def trace_steps(hand):
    os.environ["PIANOSIM_HAND"] = hand
    L = lib.load()
    L.ps_debug_qtrace.argtypes = [C.c_void_p] * 5
    L.ps_debug_qtrace.restype = C.c_int
    g = dp.BatchedPianoEnv(N, song(dp, NAME), dp.TaskConfig(trim_silence=NAME != "twinkle", **tool_hand_kwargs()),
                           device="cuda:0")
    g.reset()
    g.set_state({"t_idx": (np.arange(N) % g.song.T).astype(np.int32)})  # bench.py's stagger
    gen = torch.Generator(device="cuda:0").manual_seed(12345)
    dims = np.zeros(2, np.int32)
    steps = []
    for s in range(WARM + STEPS):
        g.step(torch.rand(N, g.action_dim, device="cuda:0", generator=gen) * 2 - 1)
        if s < WARM:
            continue
        lib.check(L.ps_debug_qtrace(g._h, dims.ctypes.data, None, None, None))
        chunks, grid = int(dims[0]), int(dims[1])
        items = np.zeros((chunks, N, 4), np.uint64)
        exits = np.zeros((grid, 2), np.uint64)
        rank = np.zeros(N, np.int32)
        lib.check(L.ps_debug_qtrace(g._h, None, items.ctypes.data, exits.ctypes.data, rank.ctypes.data))
        steps.append((items, exits, rank))
    g.close()
    return steps


def tables(steps):
    """Per step -> dict of arrays; the caller averages them."""
    rows = []
    for items, exits, rank in steps:
        chunks, n, _ = items.shape
        grid = exits.shape[0]
        ran = items[:, :, 1] != 0  # [chunks][n]
        t0 = items[:, :, 0][ran].min()
        turn, begin, end = [(items[:, :, k].astype(np.int64) - int(t0)) * US for k in range(3)]
        ticket = (items[:, :, 3] >> np.uint64(32)).astype(np.uint32).astype(np.int32)
        wg = (items[:, :, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        leave = (exits[:, 0].astype(np.int64) - int(t0)) * US
        T = leave.max()
        run = np.where(ran, end - begin, 0.0)
        cont = ran[1:]  # continuation chunks that ran
        wait = np.where(cont, begin[1:] - end[:-1], 0.0)
        own = cont & (ticket[1:] < 0)
        nlast = ran.sum(axis=0) - 1  # index of the env's last chunk
        idx = np.arange(n)
        last_begin, last_end = begin[nlast, idx], end[nlast, idx]
        dec = np.minimum(rank.astype(np.int64) * DEC // n, DEC - 1)
        r = dict(T=T, occupancy=run.sum() / (grid * T), idle=(T - leave).sum() / 1e3, idle_frac=(T - leave).sum() / (grid * T),
                 first_exit=leave.min(), p50_exit=np.median(leave), empty=float(exits[:, 1].sum()),
                 empty_max=float(exits[:, 1].max()), own_frac=own.sum() / max(cont.sum(), 1))
        r["dec"] = np.array([[run[:, dec == d].sum(axis=0).mean(), wait[:, dec == d].sum(axis=0).mean(),
                              wait[:, dec == d].sum(axis=0).max(), own[:, dec == d].sum() / max(cont[:, dec == d].sum(), 1),
                              last_begin[dec == d].mean(), last_end[dec == d].mean(), last_end[dec == d].max()]
                             for d in range(DEC)])
        # chunk boundaries: end of a chunk to the beginning of the next item on the same workgroup
        f = ran.ravel()
        w, b, e, k = wg.ravel()[f], begin.ravel()[f], end.ravel()[f], ticket.ravel()[f]
        o = np.lexsort((b, w))
        w, b, e, k = w[o], b[o], e[o], k[o]
        same = w[1:] == w[:-1]
        gap, popped = (b[1:] - e[:-1])[same], (k[1:] >= 0)[same]
        r["gap"] = np.array([gap[popped].mean() if popped.any() else 0.0, np.median(gap[popped]) if popped.any() else 0.0,
                             np.percentile(gap[popped], 99) if popped.any() else 0.0, popped.sum(),
                             gap[~popped].mean() if (~popped).any() else 0.0, (~popped).sum()])
        r["chunk_run"] = np.array([run[c][ran[c]].mean() for c in range(chunks)])
        rows.append(r)
    return {k: np.mean([r[k] for r in rows], axis=0) for k in rows[0]}


def report(hand):
    steps = trace_steps(hand)
    chunks, grid = steps[0][0].shape[0], steps[0][1].shape[0]
    t = tables(steps)
    print(f"## {hand} hand, {NAME}, {N} envs, {chunks} chunks on {grid} workgroups, {Path(lib.LIB_PATH).name}: "
          f"means of {STEPS} steps; times in us from the first pop of the launch")
    print(f"launch ends (last workgroup exit) {t['T']:.0f}; first exit {t['first_exit']:.0f}, median exit {t['p50_exit']:.0f}")
    print(f"slot occupancy (chunk run time / grid x launch) {t['occupancy']:.3f}; idle slot-time before the end "
          f"{t['idle']:.1f} slot-ms = {t['idle_frac']:.3f} of grid x launch")
    print(f"mean chunk run time by chunk: {' '.join(f'{x:.0f}' for x in t['chunk_run'])}")
    print(f"continuations run by their own workgroup {t['own_frac']:.3f}; tickets that held no item per launch "
          f"{t['empty']:.0f} (most by one workgroup {t['empty_max']:.0f})")
    print("rank decile | env run | queue wait: mean, max | self-run | last chunk: begins, ends (mean), ends (max)")
    for d, row in enumerate(t["dec"]):
        print(f"{d:11d} | {row[0]:7.0f} | {row[1]:10.0f} {row[2]:7.0f} | {row[3]:8.3f} | {row[4]:8.0f} {row[5]:8.0f} {row[6]:8.0f}")
    gp = t["gap"]
    print(f"chunk boundary (end of a chunk to the next item's begin, same workgroup): popped mean {gp[0]:.1f} "
          f"median {gp[1]:.1f} p99 {gp[2]:.1f} ({gp[3]:.0f} per launch); self-run mean {gp[4]:.1f} ({gp[5]:.0f} per launch)")
    print(flush=True)


if __name__ == "__main__":
    print(f"# tools/queue_trace.py {N} {HAND} {NAME}")
    for h in (["hull", "authored"] if HAND == "both" else [HAND]):
        report(h)
