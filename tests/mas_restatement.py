"""Monotonic alignment search (Glow-TTS, Kim et al. 2020, section 2.3 / Algorithm 1) restated in numpy: the contract of
dex_tts_amd/csrc/mas.hip and the CPU oracle of its tests.  Test infrastructure only.

For one utterance with a value matrix V [t_x, t_y] (fp32; the caller has multiplied it by the mask) the forward pass walks the frames
y = 0 .. t_y - 1 and, for the rows a monotonic path can occupy at y (max(0, t_x + y - t_y) <= x < min(t_x, y + 1)), replaces V in
place with

    Q[x, y] = max(cur, prev) + V[x, y]           one fp32 max, one fp32 add (no other rounding, no reassociation)
    cur  = -1e9 if x == y else Q[x, y - 1]       (the path cannot stay on a row it has not yet reached)
    prev = 0 if (x, y) == (0, 0), -1e9 if x == 0 < y, else Q[x - 1, y - 1]

where max(a, b) is b if b > a else a.  The backtrack starts at row t_x - 1 on the last frame and, for y = t_y - 1 .. 0, marks
(index, y) and moves up one row iff index != 0 and (index == y or Q[index, y - 1] < Q[index - 1, y - 1]): the comparison is strict,
so a tie stays on the row.  Each row is marked on a run of consecutive frames; the run lengths are the per-token durations.
"""
from __future__ import annotations

import numpy as np

NEG = np.float32(-1e9)


def forward(value: np.ndarray, t_x: int, t_y: int) -> np.ndarray:
    """Q of one utterance (a float32 copy of value with the reachable cells replaced), column by column."""
    q = np.array(value, dtype=np.float32, copy=True)
    for y in range(t_y):
        lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
        if lo >= hi:
            continue
        x = np.arange(lo, hi)
        cur = np.where(x == y, NEG, q[x, y - 1] if y > 0 else NEG).astype(np.float32)
        if y > 0:
            prev = np.where(x == 0, NEG, q[np.maximum(x - 1, 0), y - 1]).astype(np.float32)
        else:
            prev = np.zeros(len(x), np.float32)
        best = np.where(prev > cur, prev, cur).astype(np.float32)
        q[x, y] = best + q[x, y]                      # float32 + float32: one rounding
    return q


def backtrack(q: np.ndarray, t_x: int, t_y: int) -> np.ndarray:
    """Per-row durations (int32 [q.shape[0]]; 0 past t_x) of the path through Q."""
    dur = np.zeros(q.shape[0], np.int32)
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        dur[index] += 1
        if index != 0 and (index == y or q[index, y - 1] < q[index - 1, y - 1]):
            index -= 1
    return dur


def durations(value: np.ndarray, t_x, t_y) -> np.ndarray:
    """value [B, Tx, Ty] (or [Tx, Ty]) with per-row lengths -> durations [B, Tx] int32."""
    v = np.asarray(value, np.float32)
    one = v.ndim == 2
    v = v[None] if one else v
    t_x, t_y = np.atleast_1d(t_x), np.atleast_1d(t_y)
    out = np.stack([backtrack(forward(v[b], int(t_x[b]), int(t_y[b])), int(t_x[b]), int(t_y[b])) for b in range(v.shape[0])])
    return out[0] if one else out


def path_from_durations(dur: np.ndarray, Ty: int) -> np.ndarray:
    """[B, Tx] durations -> the dense 0/1 path [B, Tx, Ty] (int8)."""
    B, Tx = dur.shape
    end = np.cumsum(dur, 1)
    start = end - dur
    y = np.arange(Ty)[None, None, :]
    return ((y >= start[:, :, None]) & (y < end[:, :, None])).astype(np.int8)


def min_margin(value: np.ndarray, t_x: int, t_y: int) -> float:
    """The smallest |Q[i, y-1] - Q[i-1, y-1]| / max(|Q[i, y-1]|, |Q[i-1, y-1]|, 1) over the comparisons the backtrack makes: how
    far the path is from flipping under a perturbation of the values (0 for an exact tie)."""
    q = forward(value, t_x, t_y)
    index, m = t_x - 1, np.inf
    for y in range(t_y - 1, -1, -1):
        if index != 0 and index != y:
            a, b = float(q[index, y - 1]), float(q[index - 1, y - 1])
            m = min(m, abs(a - b) / max(abs(a), abs(b), 1.0))
        if index != 0 and (index == y or q[index, y - 1] < q[index - 1, y - 1]):
            index -= 1
    return m


def hashed_value(B: int, Tx: int, Ty: int) -> np.ndarray:
    """A deterministic integer-valued [B, Tx, Ty] matrix in [-3, 3] with many ties (the large golden case is generated, not stored)."""
    b, x, y = np.meshgrid(np.arange(B), np.arange(Tx), np.arange(Ty), indexing="ij")
    h = (x * 7 + y * 13 + b * 5 + (x * y) % 11 + (x // 3) * (y // 5)) % 7
    return (h - 3).astype(np.float32)
