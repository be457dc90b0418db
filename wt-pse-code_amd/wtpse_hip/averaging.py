"""Dense weight averaging (SWAD: Cha et al., "SWAD: Domain Generalization by Seeking Flat Minima", NeurIPS 2021): the running
means of every iterate on the device, and the loss-valley policy that decides which stretch of the run is averaged.

The reference's config.yaml asks for the recipe (`swad: LossValley`, `n_converge: 3`, `n_tolerance: 6`, `tolerance_ratio: 1.5`)
and nothing in it reads those keys; this module is what they configure here.

Three layers:
  * `avg_step_spec` / `avg_merge_spec`: the arithmetic of wtpse_avg_step / wtpse_avg_merge (csrc/average.hip) restated in numpy
    fp32.  The device results equal them bit for bit.
  * `WeightAverage`: the device state of the CURRENT segment (the mean of the iterates since the last evaluation): one flat fp32
    buffer per network, a device count, a device gate.  One recordable call per step folds all networks.
  * `LossValley`: the policy — host logic over scalars and opaque segment handles, testable without a GPU.
"""
import numpy as np

MAX_SEGMENT = 1 << 24        # (float)k is exact up to here: the longest segment wtpse_avg_step may fold


# ------------------------------------------------------------------------------------------------ specification
def avg_step_spec(a, p, k):
    """What wtpse_avg_step leaves in `a` when it folds the k-th iterate p (k = count + 1 >= 1): p itself for k == 1 (whatever a
    held), else a + (p - a) / (float)k with subtraction, division and addition each rounded to fp32.  -> a new fp32 array."""
    p = np.asarray(p, dtype=np.float32)
    if int(k) == 1:
        return p.copy()
    a = np.asarray(a, dtype=np.float32)
    d = np.subtract(p, a, dtype=np.float32)
    q = np.divide(d, np.float32(int(k)), dtype=np.float32)
    return np.add(a, q, dtype=np.float32)


def avg_merge_spec(acc, seg, n_acc, n_seg):
    """wtpse_avg_merge: the mean `seg` of n_seg iterates merged into the mean `acc` of n_acc.  n_acc == 0: seg.  Otherwise
    w = (float)((double)n_seg / (double)(n_acc + n_seg)) and acc + (seg - acc) * w, multiply and add rounded separately.
    -> a new fp32 array (acc is not modified)."""
    seg = np.asarray(seg, dtype=np.float32)
    if int(n_acc) == 0:
        return seg.copy()
    acc = np.asarray(acc, dtype=np.float32)
    w = np.float32(float(int(n_seg)) / float(int(n_acc) + int(n_seg)))
    d = np.subtract(seg, acc, dtype=np.float32)
    return np.add(acc, np.multiply(d, w, dtype=np.float32), dtype=np.float32)


def _merge(acc, seg, n_acc, n_seg):
    """The default `merge` of LossValley: ops.avg_merge for device tensors (in place), avg_merge_spec for numpy arrays."""
    if isinstance(seg, np.ndarray):
        return avg_merge_spec(acc, seg, n_acc, n_seg)
    from . import ops
    return ops.avg_merge(acc, seg, n_acc, n_seg)


def _copy(x):
    return x.copy() if isinstance(x, np.ndarray) else x.clone()


# ------------------------------------------------------------------------------------------------ device state
class WeightAverage:
    """The running means of the current segment for `nets` (HipNet roots; None entries are dropped): `avg[i]`, fp32, the size of
    nets[i].flat_params(); `count` (device int32: iterates folded since the last take()); `gate` (device int32, initially 1:
    0 = update() changes nothing any more).  The buffers are allocated once; their addresses never change, so a recorded
    update() stays valid for the life of the object."""

    def __init__(self, nets):
        import torch
        self.nets = [n for n in nets if n is not None]
        if not 1 <= len(self.nets) <= 4:
            raise ValueError("WeightAverage folds one to four networks in one call, got %d" % len(self.nets))
        flats = [n.flat_params() for n in self.nets]
        self.avg = [torch.zeros_like(f) for f in flats]
        self.count = torch.zeros(1, dtype=torch.int32, device=flats[0].device)
        self.gate = torch.ones(1, dtype=torch.int32, device=flats[0].device)
        self._issued = 0          # host-side upper bound of the count (a held or gated update is counted here, not there)

    def tick(self):
        """Host bookkeeping of one executed update(): refuses a segment longer than 2^24 iterates.  update() calls it itself when
        it executes; whoever REPLAYS a recorded update() (TrainStep) calls it once per replay."""
        if self._issued >= MAX_SEGMENT:
            raise ValueError("the current segment already holds %d iterates: a segment is at most 2^24 long ((float)k must be exact); "
                             "take() it first" % self._issued)
        self._issued += 1

    def update(self, hold=None):
        """Fold the networks' current parameters into the means: ONE wtpse_avg_step call (recordable: every argument is an address
        that stays put).  hold: optional device int32 (a LossLog's flag): non-zero = nothing changes."""
        import torch
        from . import ops
        if not torch.cuda.is_current_stream_capturing():
            self.tick()
        ops.avg_step(self.avg, [n.flat_params() for n in self.nets], self.count, self.gate, hold)

    def take(self):
        """-> ([clone of every mean], count) of the segment, and the count is zeroed: the next update() starts a new segment
        (k == 1 copies, so the buffers need no clearing).  Stream-ordered; the count is read once (one small copy: synchronises)."""
        seg = [a.clone() for a in self.avg]
        count = int(self.count.item())
        self.count.zero_()
        self._issued = 0
        return seg, count

    def close_gate(self):
        """From here on update() changes neither a mean nor the count (stream-ordered write; recorded calls see it)."""
        self.gate.zero_()

    def state(self):
        """Plain data and tensors.  The means travel only while the segment holds iterates (count > 0)."""
        count = int(self.count.item())
        return {"count": count, "gate": int(self.gate.item()), "avg": [a.clone() for a in self.avg] if count > 0 else []}

    def load_state(self, state):
        """In place: a recorded update() stays valid."""
        if state["avg"]:
            if [int(a.numel()) for a in state["avg"]] != [int(a.numel()) for a in self.avg]:
                raise ValueError("the saved means hold %s elements, these networks %s"
                                 % ([int(a.numel()) for a in state["avg"]], [int(a.numel()) for a in self.avg]))
            for dst, src in zip(self.avg, state["avg"]):
                dst.copy_(src)
        self.count.fill_(int(state["count"]))
        self.gate.fill_(int(state["gate"]))
        self._issued = int(state["count"])


# ------------------------------------------------------------------------------------------------ policy
class LossValley:
    """Which evaluations' segments are averaged: SWAD's Algorithm 1 on the validation loss, over segment means.

    The specification is this project's own.  It follows Algorithm 1 of the SWAD paper; there is no copy of the SWAD code to pin
    it against, and the tolerance threshold is `tolerance_ratio x mean` of the converging window's losses, as in the paper.
    Defaults: the reference's config.yaml (n_converge 3, n_tolerance 6, tolerance_ratio 1.5).

    Evaluations are numbered e = 0, 1, ...; evaluation e delivers S_e (the mean of the iterates since the previous evaluation, an
    opaque handle: a list of tensors or arrays), their number c_e >= 1 and the loss l_e of the current weights.  With Ns =
    n_converge and Ne = n_tolerance:
      start   s = the smallest index with l_s <= l_j for all j in s .. s+Ns-1 (decidable at evaluation s+Ns-1);
              threshold T = tolerance_ratio * mean(l_s .. l_{s+Ns-1}), in float64.
      end     t = the smallest index > s with min(l_t .. l_{t+Ne-1}) > T (decidable at t+Ne-1); then `closed` is True and later
              observations are ignored.
      result  `merge` folded over S_s .. S_{t-1} in index order with their counts; a run that ends before an end is found
              covers S_s .. the last observed segment; without a start the result is the last segment alone, converged False.
    Memory: before the start the last Ns segments are held, after it at most Ne; a segment is merged into the running result as
    soon as it is known to lie inside.

    merge(acc, seg, n_acc, n_seg) -> the merged mean, called per tensor of a segment (may work in place on acc and return it):
    ops.avg_merge for device tensors, avg_merge_spec for numpy arrays (the default picks by type)."""

    def __init__(self, n_converge=3, n_tolerance=6, tolerance_ratio=1.5, merge=None):
        self.n_converge, self.n_tolerance, self.tolerance_ratio = int(n_converge), int(n_tolerance), float(tolerance_ratio)
        if self.n_converge < 1 or self.n_tolerance < 1:
            raise ValueError("n_converge and n_tolerance must be at least 1, got %d / %d" % (self.n_converge, self.n_tolerance))
        self.merge = _merge if merge is None else merge
        self.losses, self.counts, self.iterations = [], [], []
        self.start = self.end = self.threshold = None
        self.closed = False
        self._next = None          # the next end candidate: every index in [start, _next) is merged into _final
        self._held = []            # [(index, segment)] in index order: not yet known to lie inside or outside
        self._final, self._n_final = None, 0

    # ---- parameters as plain data (TrainRun.config)
    def config(self):
        return {"n_converge": self.n_converge, "n_tolerance": self.n_tolerance, "tolerance_ratio": self.tolerance_ratio}

    @property
    def held(self):
        """Number of segments currently held back."""
        return len(self._held)

    def _fold(self, final, n_final, seg, count):
        if final is None:
            return list(seg), count       # merge with n_acc == 0 copies: the segment itself becomes the running result
        return [self.merge(f, x, n_final, count) for f, x in zip(final, seg)], n_final + count

    def observe(self, segment, count, loss, iteration=None):
        """Evaluation e = len(self.losses): the segment (owned by this object from here on), its number of iterates, the loss."""
        if self.closed:
            return
        if int(count) < 1:
            raise ValueError("evaluation %d delivers a segment of %d iterates: a segment holds at least one" % (len(self.losses), count))
        e = len(self.losses)
        self.losses.append(float(loss))
        self.counts.append(int(count))
        self.iterations.append(-1 if iteration is None else int(iteration))
        self._held.append((e, list(segment)))
        Ns, Ne, l = self.n_converge, self.n_tolerance, self.losses
        if self.start is None:
            s = e - Ns + 1
            if s < 0:
                return
            if all(l[s] <= l[j] for j in range(s, e + 1)):
                self.start = s
                self.threshold = self.tolerance_ratio * float(np.mean(np.asarray(l[s:e + 1], dtype=np.float64)))
                self._next = s + 1
                self._final, self._n_final = self._fold(None, 0, self._held.pop(0)[1], self.counts[s])
            else:
                self._held.pop(0)          # S_s is no start and lies before any later one
                return
        while self._next + Ne - 1 <= e:
            t = self._next
            if min(l[t:t + Ne]) > self.threshold:
                self.end, self.closed = t, True
                self._held = []
                return
            i, seg = self._held.pop(0)
            assert i == t
            self._final, self._n_final = self._fold(self._final, self._n_final, seg, self.counts[t])
            self._next = t + 1

    def result(self):
        """-> (tensors, info): the averaged weights as the run stands (nothing here is modified: an open valley's held segments are
        merged into a copy) and {"converged", "start", "end", "iterates", "threshold", "losses", "iterations", "evaluations"}."""
        if not self.losses:
            raise ValueError("no evaluation has been observed: there is nothing to average")
        if self.start is None:
            i, seg = self._held[-1]
            tensors, n = [_copy(x) for x in seg], self.counts[i]
        else:
            tensors, n = [_copy(x) for x in self._final], self._n_final
            for i, seg in self._held:
                tensors, n = self._fold(tensors, n, seg, self.counts[i])
        info = {"converged": self.start is not None, "start": self.start, "end": self.end, "iterates": int(n),
                "threshold": self.threshold, "losses": list(self.losses), "iterations": list(self.iterations),
                "evaluations": len(self.losses)}
        return tensors, info

    def table(self):
        """One row per evaluation: [evaluation, iteration, loss, "held" | "merged" | "outside"]."""
        held = {i for i, _ in self._held}
        rows = []
        for e, (it, loss) in enumerate(zip(self.iterations, self.losses)):
            if e in held:
                status = "held"
            elif self.start is not None and self.start <= e < self._next:
                status = "merged"
            else:
                status = "outside"
            rows.append([e, it, loss, status])
        return rows

    def state(self):
        """Plain data and the held / merged segments themselves (tensors or arrays, not copied)."""
        return {"config": self.config(), "losses": list(self.losses), "counts": list(self.counts), "iterations": list(self.iterations),
                "start": self.start, "end": self.end, "threshold": self.threshold, "closed": bool(self.closed), "next": self._next,
                "held_index": [i for i, _ in self._held], "held": [list(seg) for _, seg in self._held],
                "final": list(self._final) if self._final is not None else [], "n_final": int(self._n_final)}

    def load_state(self, state, device=None):
        """device: where tensor segments are to live (a checkpoint read with map_location="cpu" hands them over in host memory)."""
        def _copy(x):
            return x.copy() if isinstance(x, np.ndarray) else x.clone() if device is None else x.to(device, copy=True)
        if dict(state["config"]) != self.config():
            raise ValueError("the saved valley was run with %s, this one has %s" % (dict(state["config"]), self.config()))
        self.losses, self.counts = [float(v) for v in state["losses"]], [int(v) for v in state["counts"]]
        self.iterations = [int(v) for v in state["iterations"]]
        self.start, self.end, self.threshold = state["start"], state["end"], state["threshold"]
        self.closed, self._next = bool(state["closed"]), state["next"]
        self._held = [(int(i), [_copy(x) for x in seg]) for i, seg in zip(state["held_index"], state["held"])]
        self._final = [_copy(x) for x in state["final"]] if state["final"] else None
        self._n_final = int(state["n_final"])
