"""NumPy reference of the reference's ControlTestCallback bookkeeping (neural/callbacks.py:90-119), for the tests of
b747_ppo_track_best and ppo.ControlTest: a straight transcription -- Python lists, `[-W:]`, np.mean,
strict `>` -- one tracker per member.

`track` takes what the callback's calc_stepinfo computes per evaluation (the [P, R] per-reference settling_time,
|overshoot| and quality) or, with `last`, the per-evaluation means themselves (so that a test can drive the reference
from the kernel's own `last` and hold everything downstream to equality), and how often each evaluation is booked.
`track_deque` is a second, collections.deque-based restatement; `mean8` is the summation order include/b747.h
describes, which np.mean follows for up to 128 values."""
import collections

import numpy as np

METRICS = ("settling_time", "overshoot", "quality")


def quality(itse, vref, tk):
    """Controller.quality (core/controller.py:336) / evaluate.quality on float64 arrays"""
    itse, vref = np.asarray(itse, dtype=np.float64), np.asarray(vref, dtype=np.float64)
    return np.exp(-60 * 0.1 * itse / (tk * vref ** 2))


def means(metrics):
    """[P, 3] the callback's np.mean(times), np.mean(overshoots), np.mean(qualities) from metrics [3][P][R] (lists)"""
    return np.array([[np.mean([float(v) for v in metrics[m][p]]) for m in range(3)] for p in range(len(metrics[0]))],
                    dtype=np.float64)


class _Callback:
    """One member's ControlTestCallback state, as the reference keeps it"""

    def __init__(self, window):
        self.window_length = window
        self.infos = {k: [] for k in METRICS}
        self.best_mean_quality = self.mean_quality = 0
        self.n_pushes, self.best_eval = 0, -1
        self.window_mean = [np.nan] * 3

    def push(self, last):
        """calc_stepinfo's tail (lines 91-97) and _on_step's comparison (lines 113-119); True where the model is saved"""
        for k, v in zip(METRICS, last):
            self.infos[k].append(v)
        for k in METRICS:
            self.infos[k] = self.infos[k][-self.window_length:]
        self.window_mean = [np.mean(self.infos[k]) for k in METRICS]
        self.mean_quality = self.window_mean[2]
        self.n_pushes += 1
        if self.mean_quality > self.best_mean_quality:
            self.best_mean_quality = self.mean_quality
            self.best_eval = self.n_pushes - 1
            return True
        return False


def track(last_per_call, repeats, window):
    """last_per_call: per call a [P, 3] array of the evaluation's means; repeats: per call how often it is booked.
    Returns per call a dict: last [P, 3], window_mean [P, 3], best_quality [P], best_eval [P], count [P], saved [P]
    (bool: the member's model was saved in this call), margin [P] (the smallest |window_mean.quality - best so far|
    over the call's decisions; NaN where the windowed quality is NaN)."""
    P = len(last_per_call[0])
    cbs = [_Callback(window) for _ in range(P)]
    out = []
    for last, rep in zip(last_per_call, repeats):
        saved, margin = [False] * P, [np.inf] * P
        for p, cb in enumerate(cbs):
            for _ in range(rep):
                before = cb.best_mean_quality
                saved[p] |= cb.push([float(v) for v in last[p]])
                margin[p] = min(margin[p], abs(cb.mean_quality - before)) if cb.mean_quality == cb.mean_quality \
                    else margin[p]
        out.append({"last": np.array(last, dtype=np.float64),
                    "window_mean": np.array([cb.window_mean for cb in cbs], dtype=np.float64),
                    "best_quality": np.array([cb.best_mean_quality for cb in cbs], dtype=np.float64),
                    "best_eval": np.array([cb.best_eval for cb in cbs], dtype=np.int64),
                    "count": np.array([cb.n_pushes for cb in cbs], dtype=np.int64),
                    "saved": np.array(saved), "margin": np.array(margin, dtype=np.float64)})
    return out


def ring(last_per_call, repeats, window):
    """[3, P, W] what the kernel's ring holds after the calls: push k of a member in slot k % W (NaN where never
    written)"""
    P = len(last_per_call[0])
    r = np.full((3, P, window), np.nan)
    k = 0
    for last, rep in zip(last_per_call, repeats):
        for _ in range(rep):
            r[:, :, k % window] = np.asarray(last, dtype=np.float64).T
            k += 1
    return r


def track_deque(last_per_call, repeats, window):
    """`track`'s window_mean, best_quality and best_eval per call, restated with collections.deque(maxlen=window)"""
    P = len(last_per_call[0])
    wins = [[collections.deque(maxlen=window) for _ in range(3)] for _ in range(P)]
    best, best_eval, n = [0.0] * P, [-1] * P, 0
    out = []
    for last, rep in zip(last_per_call, repeats):
        wm = np.full((P, 3), np.nan)
        for r in range(rep):
            for p in range(P):
                for m in range(3):
                    wins[p][m].append(float(last[p][m]))
                    wm[p, m] = np.mean(list(wins[p][m]))
                if wm[p, 2] > best[p]:
                    best[p], best_eval[p] = wm[p, 2], n + r
        n += rep
        out.append({"window_mean": wm, "best_quality": np.array(best), "best_eval": np.array(best_eval)})
    return out


def mean8(a):
    """The mean of the sequence a in the order include/b747.h gives for b747_ppo_track_best (plain Python floats)"""
    a = [float(x) for x in a]
    n = len(a)
    if n < 8:
        s = 0.0
        for x in a:
            s += x
        return s / n
    r = a[:8]
    full = n - n % 8
    for i in range(8, full, 8):
        for j in range(8):
            r[j] += a[i + j]
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[full:]:
        s += x
    return s / n


def same(a, b):
    """Elementwise equality with NaN positions equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))
