"""float64 restatement of the three weight-averaging rules of tensorflow-addons 0.12+ that `--average_type` selects
(common/model_utils.py:133-172): MovingAverage, SWA and Lookahead.  It is the checker of tests/test_avg_optimizer_*.py,
written from the rules as DESIGN.md states them -- neither tensorflow nor tensorflow-addons is needed.

t is the 1-based count of optimiser steps since the optimiser object was new (tfa's `iterations` inside the averaging op
is t - 1); w is the weight AFTER the wrapped optimiser's own update of step t.  Entries where `active` is False have no
slot: nothing happens to them.
"""
import numpy as np


def swa_snapshot(t, start=0, period=10):
    """-> the number of snapshots already averaged if step t takes one, else None"""
    it = t - 1
    ns = max(0, (it - start) // period)
    return ns if (it >= start and it == start + ns * period) else None


def lookahead_syncs(t, sync_period=6):
    return t % sync_period == 0


def ema_step(avg, w, decay=0.99, active=None):
    avg, w = np.asarray(avg, np.float64), np.asarray(w, np.float64)
    new = avg - (avg - w) * (1.0 - decay)
    return new if active is None else np.where(active, new, avg)


def swa_step(avg, w, t, start=0, period=10, active=None):
    avg, w = np.asarray(avg, np.float64), np.asarray(w, np.float64)
    ns = swa_snapshot(t, start, period)
    if ns is None:
        return avg
    new = (avg * ns + w) / (ns + 1.0)
    return new if active is None else np.where(active, new, avg)


def lookahead_step(slow, w, t, sync_period=6, alpha=0.5, active=None):
    """-> (slow, w) after step t; on a sync step both are slow + alpha * (w - slow)"""
    slow, w = np.asarray(slow, np.float64), np.asarray(w, np.float64)
    if not lookahead_syncs(t, sync_period):
        return slow, w
    sb = slow + alpha * (w - slow)
    if active is None:
        return sb, sb
    return np.where(active, sb, slow), np.where(active, sb, w)


class Averager:
    """one rule over a run: feed it the observed post-update weights step by step"""

    def __init__(self, kind, init, active=None, **kw):
        assert kind in ('ema', 'swa', 'lookahead')
        self.kind, self.kw, self.active = kind, kw, active
        self.avg = np.asarray(init, np.float64).copy()
        self.t = 0

    def step(self, w):
        """w: the weights after the wrapped optimiser's update of the next step -> the slot after that step"""
        self.t += 1
        if self.kind == 'ema':
            self.avg = ema_step(self.avg, w, active=self.active, **self.kw)
        elif self.kind == 'swa':
            self.avg = swa_step(self.avg, w, self.t, active=self.active, **self.kw)
        else:
            self.avg, _ = lookahead_step(self.avg, w, self.t, active=self.active, **self.kw)
        return self.avg
