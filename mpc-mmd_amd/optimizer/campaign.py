"""Cutting the lockstep log of a scene-queue campaign into per-scene episodes.

A campaign (``CEM.run_campaign``) logs one row per (lockstep tick, slot); its schedule, one row per
scene -- slot, first lockstep tick, ticks run, end reason -- says which rows are whose.  ``cut`` is
a pure function of the two: no GPU, no library.
"""
from __future__ import annotations

import numpy as np

SLOT, FIRST, TICKS, REASON = range(4)                     # columns of sched (_native.QUEUE_SCHED)
UNFINISHED, COLLISION, GOAL, TICK_LIMIT = range(4)        # sched[:, REASON] (_native.QUEUE_REASONS)


def lockstep_ticks(sched):
    """The lockstep ticks the schedule's scenes have used so far: one past the last row any scene owns."""
    sched = np.asarray(sched).reshape(-1, 4)
    started = sched[:, SLOT] >= 0
    return int((sched[started, FIRST] + sched[started, TICKS]).max()) if started.any() else 0


def cut(log, sched, ticks_per_episode):
    """log: {name: array [T, E, ...]} of lockstep rows; sched [N, 4].  Returns {name: array
    [ticks_per_episode, N, ...]}: scene i's rows log[name][first:first + ticks, slot] at [:ticks, i],
    the rows after them repeating its last row (zeros for a scene with no row), as the rows after an
    episode's end repeat its frozen state; plus end_tick [N] (the local tick of a scene's last row,
    -1 without one), end_reason [N] and done_tick [N] (end_tick where the episode ended by a
    collision or the goal, else -1: ``run_episodes``' convention)."""
    sched = np.asarray(sched, np.int64).reshape(-1, 4)
    N, Tp = sched.shape[0], int(ticks_per_episode)
    out = {}
    for name, a in log.items():
        a = np.asarray(a)
        T, E = a.shape[:2]
        o = np.zeros((Tp, N) + a.shape[2:], a.dtype)
        for i, (slot, first, n, _) in enumerate(sched):
            if slot < 0 or n < 1:
                continue
            if slot >= E or first < 0 or n > Tp or first + n > T:
                raise ValueError(f"scene {i}: rows {first}..{first + n - 1} of slot {slot} are not in a log of "
                                 f"{T} ticks x {E} slots (or exceed {Tp} ticks per episode)")
            o[:n, i] = a[first:first + n, slot]
            o[n:, i] = a[first + n - 1, slot]
        out[name] = o
    ran = sched[:, SLOT] >= 0
    out["end_tick"] = np.where(ran, sched[:, TICKS] - 1, -1).astype(np.int32)
    out["end_reason"] = sched[:, REASON].astype(np.int32)
    ended = (out["end_reason"] == COLLISION) | (out["end_reason"] == GOAL)
    out["done_tick"] = np.where(ended, out["end_tick"], -1).astype(np.int32)
    return out
