"""Extra terms of the objective of calls A and C (step.py): what every term shares.  `WeightSchedule` is the base of a term's
schedule class (boundary.BoundaryLoss, overlap.OverlapLoss, lovasz.LovaszLoss); `LossTerm` is one term of a TrainStep that is switched on.  Which terms
exist, in which order they are issued and named, says the table step.TERMS."""
import math

import torch


class WeightSchedule:
    """weight_at(epoch) = min(cap, weight + ramp * epoch); cap None: no cap.  A subclass validates its own arguments with `_nonneg`
    (one that has no "no cap" form passes cap through it, which refuses None) and sets weight, ramp and cap."""

    @classmethod
    def _nonneg(cls, **values):
        for name, v in values.items():
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError("%s: %s must be a finite number >= 0, got %r" % (cls.__name__, name, v))

    def weight_at(self, epoch):
        w = self.weight + self.ramp * int(epoch)
        return w if self.cap is None else min(self.cap, w)


class LossTerm:
    """One term of a TrainStep: key (the constructor keyword and the stem of the state key `<key>_weight`), tag (its scalar is
    `<tag>_od` / `<tag>_oc` in the result and in the log), the user's schedule object, the weight as last set on the host (`weight`)
    and as the one device float the kernel reads (`dev`; starts at schedule.weight_at(0))."""

    def __init__(self, key, tag, schedule, issue, device):
        self.key, self.tag, self.schedule, self._issue = key, tag, schedule, issue
        self.weight = float(schedule.weight_at(0))
        self.dev = torch.full((1,), self.weight, dtype=torch.float32, device=device)

    def issue(self, out, target, mask, dx):
        """The term of one call: -> its unweighted value (0-dim device fp32); adds the weight's share of its gradient into dx."""
        return self._issue(self, out, target, mask, dx)

    def set_weight(self, w):
        """From the next step on, recorded or not: a stream-ordered write of the device float (rounded to fp32), no host sync."""
        w = float(w)
        if not (w >= 0.0 and w != float("inf")):
            raise ValueError("the %s weight must be a finite number >= 0, got %r" % (self.key, w))
        self.weight = w
        self.dev.fill_(w)
