"""The training run: counterpart of the reference's Trainer.train() / train_epoch() (Trainer.py:729-1060) around
`step.py::TrainStep` — epochs, the per-epoch loss sums, the NaN stop, the learning-rate schedule, validation every N epochs,
checkpoints a run can be continued from.

What differs from the reference loop, and why it cannot change a result:
  * no host synchronisation inside an epoch.  The reference reads every loss of every iteration with `.item()` (eleven times per
    iteration) for its running sums and its NaN test; here one single-wave launch per update() call folds the call's loss scalars
    into device doubles and evaluates the NaN test (wtpse_loss_log), and the host reads sums and flag ONCE per epoch.  A double
    accumulator fed in iteration order holds the reference's running sums bit for bit.
  * the NaN stop.  The reference raises before backward(); a run that never synchronises cannot, so the flag the NaN test raises
    holds every later Adam launch (wtpse_adam_dev's `hold`): from the failing iteration on no parameter and no Adam moment
    changes, and `train_epoch()` raises the reference's ValueError, naming the iteration, when it reads the log.  The flag is read
    before every validation and before every file this module writes: nothing is ever written from a poisoned run.
  * averaged weights (SWAD; `TrainRun(swad=...)`, off by default).  The one exception to "no host synchronisation inside an epoch":
    every `swad_every`-th iteration the run stops at ONE point to evaluate — it reads the NaN flag, the loss of the current weights and
    the count of the segment it takes (three small copies at the same point; the first one drains the stream) — and goes on.  Between
    evaluations the running means are kept by one more launch per step (wtpse_avg_step, part of the recorded step), with no host
    contact.  Once the loss valley is closed no further evaluation runs.
  * no tensorboard scalars, image grids, `code/` snapshot or yaml dump.

Data-parallel runs are not covered here (`TrainStep`'s own `dp` path is).
"""
import csv
import os
import random
import time
from bisect import bisect_right

import numpy as np
import torch

from . import ops
from .averaging import LossValley, WeightAverage
from .step import NET_KEYS, TERMS, TrainStep
from .validate import best_checkpoint, eval_mode, predict_pair

CKPT_KEYS = ("model", "model_shape", "model_oc", "model_oc_shape")     # Trainer.py:282-288, in the order (od, od_shape, oc, oc_shape)


def reference_lr(epoch, max_epoch, base_lr, warmup_factor=0.001, steps=(100, 150), gamma=0.5):
    """Trainer.lr_update's arithmetic (Trainer.py:989-1004 with the constants of :1016-1021) in Python floats: the rate that
    applies after `epoch` has been trained.  Quirks kept:
      * `warmup_steps = 2 * max_epoch`: alpha = epoch / (2 * max_epoch) never reaches 1 inside a run, so the warm-up never
        completes — at the last epoch the factor is still about one half;
      * the reference gives the shape networks the SEGMENTATION networks' base rates (lr for optim_shape, lr_oc for
        optim_shape_oc), not lr_shape / lr_oc_shape: `TrainRun(lr_schedule="reference")` does the same."""
    alpha = epoch / (max_epoch * 2)
    wf = warmup_factor * (1 - alpha) + alpha
    return base_lr * wf * gamma ** bisect_right(steps, epoch)


class LossLog:
    """Device-side running sums of a step's losses plus the NaN flag (wtpse_loss_log): `acc` float64 [len(names)] and `flag`
    int32 [2] = (raised, iteration) share one allocation, so read() is one device-to-host copy."""

    def __init__(self, device, names):
        self.names = list(names)
        n = len(self.names)
        self._buf = torch.zeros(n + 1, dtype=torch.float64, device=device)
        self.acc = self._buf[:n]
        self.flag = self._buf[n:].view(torch.int32)

    def read(self):
        """-> ({name: sum}, (nan, iteration)): synchronises with the stream (one copy)."""
        host = self._buf.cpu()
        n = len(self.names)
        flag = host[n:].view(torch.int32).tolist()
        return dict(zip(self.names, host[:n].tolist())), (bool(flag[0]), int(flag[1]))

    def reset(self):
        """Zero the sums (stream-ordered).  The flag is sticky: it is never cleared."""
        self.acc.zero_()


class FundusBatches:
    """`next_batch` over an on-disk dataset: Trainer.get_multi_batch (Trainer.py:29-55) on `FundusTree`s, one per source domain,
    with the per-sample transforms on the GPU (`DeviceInputPipeline`).  Per call: the domain list is shuffled with the run's
    `random.Random` (Trainer.py:769), the sample indices come from its numpy generator (fundus_dataloader.py:90), the crop draws
    from the `random.Random` again (custom_transforms.py:342-346), one sample after the other as the reference's loader does.
    The reference shuffles its domain list in place, so every shuffle starts from the order the previous one left: that order
    (`order`: positions into the datasets as they were given) is run state — `state()` / `load_state()`, which TrainRun's
    checkpoints carry — and a feed built anew from the same datasets in the same order continues a run where it stopped.

    augment: an `input_pipeline.Augment` switches the device-side augmentation stage on (None: off, and everything here is as it
    was).  The reference's loader transforms a sample right after it has drawn its index, so with augmentations — whose noise points
    and eraser draw from the numpy generator too — the draws interleave per sample: index, crop, augmentations.  The elastic
    transform's uniform fields come from the device Philox stream `noise_seed` (TrainRun sets it to the run seed: `set_seed`) at a
    running position, which is feed state as well: `state()` carries it as "noise_pos", and a state saved before the field existed
    loads with position 0.

    style, appearance, quality, jpeg, clahe: one keyword per optional stage behind the augmentations (`input_pipeline.stages`), each
    taking that stage's config — `AmplitudeMix`, `AppearanceNets`, `ImageQuality`, `JpegCompression`, `Clahe` — or None: the stage
    is off, and not one launch, allocation or draw is added.  A config of another type or one that does not take the side is a
    ValueError here.  The stages run in `stages.RUN_ORDER` and draw, from the numpy generator AFTER all of the batch's other draws,
    in `stages.DRAW_ORDER` — the order in which they were added, so that every stream is what it is without the stages behind it.
    The generator, which TrainRun's checkpoints carry, is all the state they have, with one exception.  Particular to a stage:
      * style: a batch is assembled domain-major, so every sample has partners from the other domains next to it; it needs at least
        two source domains and a side that is a power of two from 32 to 512.
      * quality: its noise comes from the device Philox stream `set_seed` sets (blocks of their own) at a running position, which is
        feed state: `state()` carries it as "quality_pos" when the stage is on, and a state saved without the field loads with
        position 0.
      * appearance (side 1 .. 512) and jpeg (a side that is a multiple of 16) are training augmentations whose effect on the Dice /
        HD95 of a held-out domain has not been measured.
      * clahe draws nothing; it is a preprocessing step, so whatever reads the run's checkpoints must apply the same one: TrainRun
        writes `clahe.record()` into every checkpoint as "clahe" (`clahe_record()` is what it asks the feed for)."""

    def __init__(self, datasets, batch_size, device, size=256, augment=None, pipe=None, style=None, quality=None, clahe=None,
                 appearance=None, jpeg=None):
        from .input_pipeline import DeviceInputPipeline
        from .input_pipeline.stages import RUN_ORDER
        self.augment = augment
        self.datasets = list(datasets)
        if style is not None and len(self.datasets) < 2:
            raise ValueError("amplitude mixing needs at least two source domains, got %d" % len(self.datasets))
        given = {"style": style, "appearance": appearance, "quality": quality, "jpeg": jpeg, "clahe": clahe}
        for stage in RUN_ORDER:
            config = given[stage.feed_kw]
            if config is not None:
                if not isinstance(config, stage.config):
                    raise ValueError("%s must be an input_pipeline.%s or None, got %r" % (stage.feed_kw, stage.config.__name__, config))
                stage.check_size(int(size), config)
            setattr(self, stage.feed_kw, config)
        self.order = list(range(len(self.datasets)))
        # Trainer.py:1011: per_domain_batch = batch_size // source_domain_num — a batch holds domains * per_domain samples
        # (30 for the reference's batch_size 32 over three source domains)
        self.batch_size = int(batch_size)
        self.per_domain = self.batch_size // len(self.datasets)
        if self.per_domain < 1:
            raise ValueError("batch_size %d is smaller than the number of source domains (%d)" % (batch_size, len(self.datasets)))
        self.size = int(size)
        self.pipe = DeviceInputPipeline(size, device) if pipe is None else pipe     # pipe: a ready pipeline of the same size

    def __len__(self):
        """Trainer.py:1013-1014: iterations per epoch = total samples // batch size."""
        return sum(len(d) for d in self.datasets) // self.batch_size

    def __call__(self, py_rng, np_rng):
        from .fundus_data import multi_batch
        from .input_pipeline import draw, draw_augment
        py_rng.shuffle(self.order)
        if self.augment is None:
            images, masks = multi_batch([self.datasets[i] for i in self.order], self.per_domain, np_rng)
            draws = [draw(py_rng, self.size) for _ in images]
            return self.pipe(images, masks, draws, **self._stage_draws(np_rng, len(images)))
        images, masks, draws, aug_draws = [], [], [], []
        for i in self.order:
            for _ in range(self.per_domain):
                img, mask = multi_batch([self.datasets[i]], 1, np_rng)
                images += img
                masks += mask
                draws.append(draw(py_rng, self.size))
                aug_draws.append(draw_augment(py_rng, np_rng, self.size, self.augment))
        return self.pipe(images, masks, draws, aug_draws, **self._stage_draws(np_rng, len(images)))

    def _stage_draws(self, np_rng, n):
        """The pipeline keywords of the stages that are on, drawn in `stages.DRAW_ORDER` (which says why it is not the run order)."""
        from .input_pipeline.stages import DRAW_ORDER
        return {stage.pipe_kw: stage.draw(np_rng, n, self) for stage in DRAW_ORDER if getattr(self, stage.feed_kw) is not None}

    def clahe_record(self):
        """The feed's preprocessing as a checkpoint carries it: `Clahe.record()`, or None without the stage."""
        return None if self.clahe is None else self.clahe.record()

    def set_seed(self, seed):
        """The seed of the device noise stream — the elastic transform's fields and the image-quality stage's noise (TrainRun calls
        this with the run seed)."""
        self.pipe.noise_seed = int(seed)

    def state(self):
        state = {"order": list(self.order)}
        if self.augment is not None:
            state["noise_pos"] = int(self.pipe.noise_pos)
        if self.quality is not None:
            state["quality_pos"] = int(self.pipe.quality_pos)
        return state

    def load_state(self, state):
        order = [int(i) for i in state["order"]]
        if sorted(order) != list(range(len(self.datasets))):
            raise ValueError("the saved domain order %s is not a permutation of this feed's %d datasets" % (order, len(self.datasets)))
        self.order = order
        self.pipe.noise_pos = int(state.get("noise_pos", 0))
        self.pipe.quality_pos = int(state.get("quality_pos", 0))


def _clahe_record_of(feed):
    """A feed, or a bound method of one (`ClaheTestBatches(...).triples`) -> (it can tell, its `clahe_record()`).  A plain
    test_run.FundusTestBatches can tell too: it applies none."""
    from .test_run import FundusTestBatches
    owner = getattr(feed, "__self__", feed)
    if owner is not None and hasattr(owner, "clahe_record"):
        return True, owner.clahe_record()
    return isinstance(owner, FundusTestBatches), None


def _py_state_to_lists(state):
    version, words, gauss = state
    return [int(version), [int(w) for w in words], -1.0 if gauss is None else float(gauss), gauss is not None]


def _py_state_from_lists(s):
    return (int(s[0]), tuple(int(w) for w in s[1]), float(s[2]) if s[3] else None)


def _np_state_to_lists(state):
    name, keys, pos, has_gauss, cached = state
    return [str(name), torch.from_numpy(np.asarray(keys, dtype=np.int64)), int(pos), int(has_gauss), float(cached)]


def _np_state_from_lists(s):
    return (str(s[0]), np.asarray(s[1].tolist(), dtype=np.uint32), int(s[2]), int(s[3]), float(s[4]))


class TrainRun:
    """Trainer.train() for the four networks of train.py:91-138.

    next_batch(py_rng, np_rng) -> (image [B,3,H,W], target_od [B,1,H,W], target_oc [B,1,H,W]) device fp32; the run owns the two
    host generators (`random.Random(seed)`: crop draws and the per-iteration shuffle of the domain list; `numpy.random.
    RandomState(seed)`: sample indices) and hands them to every call.  A feed that keeps state of its own between calls exposes it
    as `state()` -> plain data / `load_state(state)` (`FundusBatches`: the order of its domain list and, with augmentations, the
    position of its noise stream); a feed that draws device noise of its own exposes `set_seed(seed)`, which the constructor
    calls with the run seed (`FundusBatches`: the elastic transform's stream); checkpoints carry the state, so a
    resumed run draws what the uninterrupted one would.
    lr: the four base rates (od, od_shape, oc, oc_shape) or one for all.  lr_schedule: None (the reference's default: its call of
    lr_update is commented out, Trainer.py:1040) or "reference" (`reference_lr` after every epoch, from the next epoch on).
    val_batches: a sequence, or a callable returning an iterable, of (image, label_od, label_oc); validator: a `validate.Validator`.
    checkpoint_every: write out_dir/run_checkpoint.pth.tar after every that many epochs (0: never).
    freeze_bn: train on frozen BatchNorm statistics (TrainStep(freeze_bn=True)): train_epoch() keeps the networks in eval mode, the
    running statistics never change.  Part of config(), so load() restores it; a checkpoint from before the flag loads as False.
    swad: an `averaging.LossValley` switches dense weight averaging on (None, the default: off — not one launch, allocation or host
    read is added).  The step then keeps the running mean of every iterate since the last evaluation on the device
    (`averaging.WeightAverage`), and after every `swad_every`-th iteration of the run (> 0) train_epoch() evaluates: check() for the NaN
    flag, the loss of the CURRENT weights in eval mode, `average.take()`, `swad.observe(...)`, `close_gate()` once the valley is
    closed (no evaluation runs after that), and the networks go back to their training mode.
    swad_loss(run) -> float: the loss of an evaluation.  Default: over `swad_batches` — a sequence, or a callable returning an iterable,
    of (image, target_od, target_oc) in the training format at the network's size — the mean of bce_sigmoid_fwd(disc logits,
    target_od) + bce_sigmoid_fwd(cup logits, target_oc) on `validate.predict_pair`'s logits (the cup's behind the ROI mask), summed
    on the device and read once.  One of the two must be given.
    train() ends by writing out_dir/swad_checkpoint.pth.tar (`averaged_checkpoint()`) and out_dir/swad.csv; config() carries the
    valley's parameters and swad_every, state() / restore() the WeightAverage's and the LossValley's state: a resumed run writes the
    same swad_checkpoint bit for bit.  A checkpoint from before the field loads with swad off; one that carries swad state is refused
    by a run without swad.
    Extra terms of calls A and C (step.TERMS; TrainStep's docstring says how a term is issued): the keyword takes the term's schedule
    object or a saved config()'s dict form of one; None, the default: off, nothing is added.  The device weight is set to the
    schedule's weight_at(epoch) at the start of every epoch and again by restore(), so a resumed run continues the schedule bit for
    bit; the loss table gets the term's two columns through the log's names, every epoch's result carries "<keyword>_weight", and the
    schedule stays readable as the attribute of the keyword's name.
    boundary: a `boundary.BoundaryLoss`; columns bd_od / bd_oc.
    overlap: an `overlap.OverlapLoss` (soft Dice / Tversky); columns ov_od / ov_oc.
    lovasz: a `lovasz.LovaszLoss` (Lovász hinge); columns lv_od / lv_oc.
    CLAHE preprocessing: a feed that has `clahe_record()` (`FundusBatches(clahe=...)`) is asked for it once; when it returns a record,
    every checkpoint the run writes — run_checkpoint, swad_checkpoint and, through `validator.clahe`, the best-Dice checkpoint —
    carries it as "clahe" (`self.clahe_record`; absent otherwise: the files are what they were).  A `val_batches` whose owner has
    `clahe_record()` too (`labelled_split.ClaheTestBatches(...).triples`), or is a plain `FundusTestBatches`, which applies none, must
    agree with the feed: ValueError otherwise.
    """

    swad, swad_every, average = None, 0, None        # averaging is off unless the constructor switches it on
    boundary = overlap = lovasz = None                      # so are the terms of step.TERMS

    def __init__(self, model_od, shape_od, model_oc, shape_oc, hparams, next_batch, iter_per_epoch, max_epoch, lr=(1e-3, 1e-3, 1e-3, 1e-3),
                 stop_epoch=-1, val_batches=None, validator=None, interval_validate=10, lr_schedule=None, out_dir=None, graph="plan",
                 seed=0, checkpoint_every=0, betas=(0.9, 0.99), freeze_bn=False, swad=None, swad_every=0, swad_batches=None, swad_loss=None,
                 boundary=None, overlap=None, lovasz=None):
        terms = dict(boundary=boundary, overlap=overlap, lovasz=lovasz)
        for key, _, cls, _ in TERMS:
            if isinstance(terms[key], dict):        # a saved config()'s form ({}: off)
                terms[key] = cls(**terms[key]) if terms[key] else None
            setattr(self, key, terms[key])
        if isinstance(swad, dict):                  # a saved config()'s form of the valley's parameters ({}: off)
            swad = LossValley(**swad) if swad else None
        if swad is not None and int(swad_every) <= 0:
            raise ValueError("swad needs swad_every > 0 (iterations between two evaluations), got %r" % (swad_every,))
        if swad is not None and swad_batches is None and swad_loss is None:
            raise ValueError("swad needs a swad_batches feed (or a swad_loss of its own) to evaluate the current weights on")
        if lr_schedule not in (None, "reference"):
            raise ValueError("lr_schedule must be None or 'reference', got %r" % (lr_schedule,))
        if (val_batches is None) != (validator is None):
            raise ValueError("validation needs both val_batches and a Validator")
        self.nets = (model_od, shape_od, model_oc, shape_oc)
        self.hp = hparams
        self.base_lr = tuple(float(r) for r in (lr if isinstance(lr, (tuple, list)) else (lr,) * 4))
        self.next_batch, self.iter_per_epoch, self.max_epoch, self.stop_epoch = next_batch, int(iter_per_epoch), int(max_epoch), int(stop_epoch)
        self.val_batches, self.validator, self.interval_validate = val_batches, validator, int(interval_validate)
        self.lr_schedule, self.out_dir, self.seed, self.checkpoint_every = lr_schedule, out_dir, int(seed), int(checkpoint_every)
        self.graph, self.betas = graph, tuple(float(b) for b in betas)
        self.freeze_bn = bool(freeze_bn)
        self.py_rng, self.np_rng = random.Random(self.seed), np.random.RandomState(self.seed)
        if hasattr(next_batch, "set_seed"):            # a feed with a device noise stream of its own (FundusBatches with augment=)
            next_batch.set_seed(self.seed)
        seen, self.clahe_record = _clahe_record_of(next_batch)
        val_seen, val_record = _clahe_record_of(val_batches)
        if seen and val_seen and val_record != self.clahe_record:
            raise ValueError("the training feed and val_batches disagree about the CLAHE preprocessing (%r against %r): the networks "
                             "would be validated on other pictures than they are trained on" % (self.clahe_record, val_record))
        if self.clahe_record is not None and validator is not None:
            validator.clahe = dict(self.clahe_record)
        device = next(model_od.parameters()).device
        self.log = LossLog(device, TrainStep.log_names(hparams, **{key: s is not None for key, s in terms.items()}))
        self.swad, self.swad_every, self.swad_batches, self.swad_loss = swad, int(swad_every) if swad is not None else 0, swad_batches, swad_loss
        self.average = None
        if swad is not None:
            full = bool(hparams['whitening'])
            self.average = WeightAverage([n for k, n in zip(NET_KEYS, self.nets) if full or k in ("od", "oc")])
        self.train_step = TrainStep(model_od, shape_od, model_oc, shape_oc, hparams, lr=self.base_lr, betas=betas, graph=graph, log=self.log,
                                    freeze_bn=self.freeze_bn, average=self.average, **terms)
        self.epoch = 0                 # epochs completed = index of the epoch train_epoch() runs next
        self.iteration = 0             # iterations completed
        self.last = None               # what the last train_epoch() returned
        self.best = [0, 0, 0, 0, 0, 0]  # the six values of the best validation so far (what train() returns)
        if out_dir is not None:
            os.makedirs(out_dir, exist_ok=True)

    # ------------------------------------------------------------------------------------------------ one epoch
    def _raise_if_nan(self, flag):
        if flag[0]:
            raise ValueError("loss is nan while training (iteration %d)" % flag[1])

    def check(self):
        """Reads the NaN flag (one small copy, synchronises) and raises the reference's error when it is set."""
        self._raise_if_nan(self.log.read()[1])

    def _set_term_weights(self):
        """Every term's device weight to its schedule's value for the epoch that runs next."""
        for t in self.train_step.terms:
            t.set_weight(t.schedule.weight_at(self.epoch))

    def train_epoch(self):
        """`iter_per_epoch` steps without a host synchronisation, then ONE read of the loss log.  Raises
        ValueError('loss is nan while training ...') naming the 0-based iteration when the NaN test of Trainer.py:794-800 / 878-885
        has held (`epoch` and `iteration` then stay where the epoch began).  -> {"epoch", "sums": {name: float}, "means": {name: sum / iter_per_epoch}, "lr": {key: rate}, "seconds"}.
        (The reference divides SOME of its sums by len(self.train_loader), the number of source domains, and prints others
        undivided, Trainer.py:974-987; that print-only quirk is not reproduced: every mean here is over the iterations.)"""
        for n in self.nets:
            if n is not None:
                n.train(not self.freeze_bn)
        start = time.perf_counter()
        self.log.reset()
        self._set_term_weights()
        for i in range(self.iter_per_epoch):
            image, target_od, target_oc = self.next_batch(self.py_rng, self.np_rng)
            self.train_step.step(image, target_od, target_oc)
            if self.swad is not None and not self.swad.closed and (self.iteration + i + 1) % self.swad_every == 0:
                self._swad_evaluate(self.iteration + i + 1)
        sums, flag = self.log.read()
        self._raise_if_nan(flag)
        self.iteration += self.iter_per_epoch
        seconds = time.perf_counter() - start
        self.last = {"epoch": self.epoch, "sums": sums, "means": {k: v / self.iter_per_epoch for k, v in sums.items()},
                     "lr": self.train_step.get_lr(), "seconds": seconds}
        self.last.update({t.key + "_weight": t.weight for t in self.train_step.terms})
        if self.out_dir is not None:
            path = os.path.join(self.out_dir, "train_log.csv")
            new = not os.path.isfile(path)
            with open(path, "a", newline="") as f:
                w = csv.writer(f)
                if new:
                    w.writerow(["epoch", "iteration"] + self.log.names + ["lr_" + k for k in NET_KEYS] + ["seconds"])
                w.writerow([self.epoch, self.iteration] + [repr(self.last["means"][k]) for k in self.log.names]
                           + [repr(self.last["lr"].get(k, "")) for k in NET_KEYS] + ["%.3f" % seconds])
        self.epoch += 1
        return self.last

    # ------------------------------------------------------------------------------------------------ averaged weights
    def _swad_default_loss(self):
        if any(n is None for n in self.nets):
            raise ValueError("the default swad loss predicts with all four networks: pass swad_loss= for a run without shape networks")
        batches = self.swad_batches() if callable(self.swad_batches) else self.swad_batches
        total = torch.zeros((), dtype=torch.float64, device=self.log.acc.device)
        n = 0
        for image, target_od, target_oc in batches:
            pred, pred_oc = predict_pair(*self.nets, image)
            total += ops.bce_sigmoid_fwd(pred, target_od.contiguous()).double()
            total += ops.bce_sigmoid_fwd(pred_oc, target_oc.contiguous()).double()
            n += 1
        if n == 0:
            raise ValueError("swad_batches is empty")
        return float(total.item()) / n

    def _swad_evaluate(self, iteration):
        """One evaluation, `iteration` iterations into the run (the one point inside an epoch at which the host waits for the device)."""
        self.check()
        with eval_mode([n for n in self.nets if n is not None]):
            loss = float(self.swad_loss(self)) if self.swad_loss is not None else self._swad_default_loss()
        segment, count = self.average.take()
        self.swad.observe(segment, count, loss, iteration)
        if self.swad.closed:
            self.average.close_gate()

    def _forward_only(self, image, target_od, target_oc):
        """The forward halves of calls A-D as TrainStep._schedule issues them, on the networks as they stand, tapes dropped: what a
        train-mode pass does to the BatchNorm running statistics and nothing else.  The teacher pass inside calls B and D runs with
        its segmentation network in eval mode, so every BatchNorm sees the batch exactly once."""
        model_od, shape_od, model_oc, shape_oc = self.nets
        image = image.contiguous()
        res, tape = model_od._forward_update(image, target_od, image, want_tape=True)
        del tape
        out = res[0]
        if shape_od is not None and self.train_step.full:
            with eval_mode([model_od]):
                _, tape = shape_od._forward_update(model_od, image, target_od, want_tape=True)
            del tape
        roi, _ = ops.roi(image, out)
        res, tape = model_oc._forward_update(roi, target_oc, roi, want_tape=True)
        del tape, res
        if shape_oc is not None and self.train_step.full:
            with eval_mode([model_oc]):
                _, tape = shape_oc._forward_update(model_oc, roi, target_oc, want_tape=True)
            del tape

    def averaged_checkpoint(self, bn_batches=None):
        """-> the four-key dict of `best_checkpoint` for the AVERAGED weights plus "swad": {converged, start, end, iterates, threshold,
        losses, iterations, evaluations} (`LossValley.result()`'s info).

        The averaged flats are copied into the live flat buffers in place (a recorded step stays valid) and the packed weights are
        refreshed; every BatchNorm's running statistics are reset and refitted over `bn_batches` (default: iter_per_epoch) train-mode,
        forward-only passes of calls A-D (`_forward_only`), batch k with the factor 1 / k — the cumulative mean over the batches, which
        is torch.optim.swa_utils.update_bn, the pass SWAD runs on its averaged model.  The batches come from `next_batch` with fresh
        generators seeded seed + 1.  A freeze_bn run trains on statistics it never writes: it keeps them (no refit).
        Afterwards everything the run owns is put back bit for bit: parameters, buffers, packed weights, Philox positions, the feed's
        state(); Adam's state and the run's two host generators are not touched at all.  Synchronises."""
        if self.swad is None:
            raise ValueError("this run does not average (TrainRun(swad=...))")
        self.check()
        tensors, info = self.swad.result()
        nets = self.average.nets
        bn_batches = self.iter_per_epoch if bn_batches is None else int(bn_batches)
        feed_state = self.next_batch.state() if hasattr(self.next_batch, "state") else None
        saved = []
        for n in nets:
            saved.append(dict(flat=n.flat_params().clone(), packed=n._packed.clone(), x3=n._x3.clone(), version=n._packed_version,
                              bufs=[b.clone() for b in n.buffers()], ctr=n._noise_ctr.clone(), momentum=n.bn_momentum,
                              modes=[(m, m.training) for m in n.modules()]))
        try:
            for n, avg in zip(nets, tensors):
                n.flat_params().copy_(avg)
                n.invalidate_packed()
                n.ensure_ready(repack=True)
            if not self.freeze_bn and bn_batches > 0:
                for n in nets:
                    n.train(True)
                    for m in n.modules():
                        if isinstance(getattr(m, "running_mean", None), torch.Tensor) and hasattr(m, "num_batches_tracked"):
                            m.running_mean.zero_()
                            m.running_var.fill_(1.0)
                            m.num_batches_tracked.zero_()
                py_rng, np_rng = random.Random(self.seed + 1), np.random.RandomState(self.seed + 1)
                for k in range(1, bn_batches + 1):
                    for n in nets:
                        object.__setattr__(n, "bn_momentum", 1.0 / k)
                    self._forward_only(*self.next_batch(py_rng, np_rng))
            d = {key: {name: v.detach().clone() for name, v in n.state_dict().items()}
                 for key, n in zip(CKPT_KEYS, self.nets) if n is not None}
            d["swad"] = info
            if self.clahe_record is not None:
                d["clahe"] = dict(self.clahe_record)
        finally:
            for n, sv in zip(nets, saved):
                object.__setattr__(n, "bn_momentum", sv["momentum"])
                for m, mode in sv["modes"]:
                    m.training = mode
                n.flat_params().copy_(sv["flat"])
                n._packed.copy_(sv["packed"])
                n._x3.copy_(sv["x3"])
                object.__setattr__(n, "_packed_version", sv["version"])
                for b, old in zip(n.buffers(), sv["bufs"]):
                    b.copy_(old)
                n._noise_ctr.copy_(sv["ctr"])
            if feed_state is not None:
                self.next_batch.load_state(feed_state)
            torch.cuda.synchronize()
        return d

    def write_swad(self):
        """out_dir/swad_checkpoint.pth.tar (averaged_checkpoint(): loads wherever a best-Dice checkpoint does) and out_dir/swad.csv
        (one line per evaluation: evaluation, iteration, loss, held / merged / outside).  Nothing is written from a poisoned run (the
        reference's ValueError) or before the first evaluation."""
        if self.swad is None or self.out_dir is None or not self.swad.losses:
            return
        d = self.averaged_checkpoint()
        path = os.path.join(self.out_dir, "swad_checkpoint.pth.tar")
        tmp = "%s.tmp%d" % (path, os.getpid())
        torch.save(d, tmp)
        os.replace(tmp, path)
        path = os.path.join(self.out_dir, "swad.csv")
        tmp = "%s.tmp%d" % (path, os.getpid())
        with open(tmp, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["evaluation", "iteration", "loss", "status"])
            w.writerows([[e, it, repr(loss), status] for e, it, loss, status in self.swad.table()])
        os.replace(tmp, path)

    # ------------------------------------------------------------------------------------------------ the run
    def train(self):
        """Trainer.py:1025-1056 in its order: train the epoch; stop when `stop_epoch == epoch` (before its validation); the
        schedule; validate when (epoch + 1) % interval_validate == 0 and epoch > 2.  -> the six best values in the reference's
        order [cup_dice, cup_hd, cup_asd, disc_dice, disc_hd, disc_asd] (zeros while no validation has improved;
        they travel with a checkpoint, so a resumed run that finds no new best returns the earlier one).  With swad, the run ends
        (also at stop_epoch) by writing the averaged checkpoint and its table (`write_swad`)."""
        for epoch in range(self.epoch, self.max_epoch):
            self.train_epoch()
            if self.stop_epoch == epoch:
                print("Stop epoch at %d" % self.stop_epoch)
                break
            if self.lr_schedule == "reference":
                od = reference_lr(epoch, self.max_epoch, self.base_lr[0])
                oc = reference_lr(epoch, self.max_epoch, self.base_lr[2])
                self.train_step.set_lr(od=od, od_shape=od, oc=oc, oc_shape=oc)
            if self.validator is not None and (epoch + 1) % self.interval_validate == 0 and epoch > 2:
                self.check()
                batches = self.val_batches() if callable(self.val_batches) else self.val_batches
                r = self.validator(epoch, *self.nets, batches)
                if r[0] == 1:
                    self.best = [float(v) for v in r[1:]]
            if self.checkpoint_every > 0 and self.out_dir is not None and (epoch + 1) % self.checkpoint_every == 0:
                self.save(os.path.join(self.out_dir, "run_checkpoint.pth.tar"))
        self.write_swad()
        return list(self.best)

    # ------------------------------------------------------------------------------------------------ checkpoints
    def config(self):
        cfg = {"lr": list(self.base_lr), "iter_per_epoch": self.iter_per_epoch, "max_epoch": self.max_epoch, "stop_epoch": self.stop_epoch,
               "interval_validate": self.interval_validate, "lr_schedule": self.lr_schedule or "", "seed": self.seed,
               "checkpoint_every": self.checkpoint_every, "graph": self.graph, "betas": list(self.betas), "freeze_bn": self.freeze_bn,
               "swad": self.swad.config() if self.swad is not None else {}, "swad_every": self.swad_every}
        for key, *_ in TERMS:           # a term's schedule in its dict form ({}: off)
            cfg[key] = getattr(self, key).config() if getattr(self, key) is not None else {}
        return cfg

    @staticmethod
    def config_kwargs(config):
        """A saved config() as constructor arguments.  A checkpoint written before `freeze_bn` existed carries no such key: it was
        trained on batch statistics and loads as freeze_bn=False."""
        cfg = dict(config)
        cfg["lr_schedule"] = cfg["lr_schedule"] or None
        cfg["lr"], cfg["betas"] = tuple(cfg["lr"]), tuple(cfg["betas"])
        cfg["freeze_bn"] = bool(cfg.get("freeze_bn", False))
        cfg["swad"] = LossValley(**cfg["swad"]) if cfg.get("swad") else None      # (a checkpoint from before the field: off)
        cfg["swad_every"] = int(cfg.get("swad_every", 0))
        for key, *_ in TERMS:
            cfg[key] = dict(cfg.get(key) or {})                 # (a checkpoint from before the field: off)
        return cfg

    def state(self):
        """Everything save() writes, as tensors, numbers, strings, lists and dicts only (torch.load(weights_only=True) reads it):
        the four networks under the best-Dice checkpoint's four keys (test_visulization.py:132-193's filtered load reads a run
        checkpoint too), TrainStep.state_dict(), epochs and iterations completed, the Validator's best and its six values, both host
        generators, the feed's own state (when `next_batch` has one), the last epoch's loss sums."""
        self.check()
        d = best_checkpoint(*self.nets) if all(n is not None for n in self.nets) else \
            {k: n.state_dict() for k, n in zip(CKPT_KEYS, self.nets) if n is not None}
        d.update(train_step=self.train_step.state_dict(), epoch=self.epoch, iteration=self.iteration, config=self.config(),
                 best_mean_dice=float(self.validator.best_mean_dice) if self.validator is not None else 0.0,
                 best_epoch=int(self.validator.best_epoch) if self.validator is not None else -1,
                 py_rng=_py_state_to_lists(self.py_rng.getstate()), np_rng=_np_state_to_lists(self.np_rng.get_state()),
                 loss_sums=dict(self.last["sums"]) if self.last is not None else {},
                 loss_names=list(self.log.names), best=list(self.best),
                 feed=self.next_batch.state() if hasattr(self.next_batch, "state") else {})
        if self.swad is not None:
            d["swad_state"] = {"average": self.average.state(), "valley": self.swad.state()}
        if self.clahe_record is not None:
            d["clahe"] = dict(self.clahe_record)
        return d

    def save(self, path):
        """Written to a temporary name beside `path` and moved into place (os.replace): a run that is killed while it writes leaves
        the previous checkpoint whole.  Refuses (the reference's ValueError) when the NaN flag is set."""
        d = self.state()
        tmp = "%s.tmp%d" % (path, os.getpid())
        torch.save(d, tmp)
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, model_od, shape_od, model_oc, shape_oc, hparams, next_batch, **kw):
        """A TrainRun that continues the run `path` was saved from: the networks (new ones, or live ones) receive the saved weights
        and buffers, the constructor arguments that save() recorded (rates, epochs, seed, ...) are the defaults of `kw`."""
        d = torch.load(path, map_location="cpu", weights_only=True)
        cfg = cls.config_kwargs(d["config"])
        cfg.update(kw)
        for key, n in zip(CKPT_KEYS, (model_od, shape_od, model_oc, shape_oc)):
            if n is not None:
                n.load_state_dict(d[key])
        run = cls(model_od, shape_od, model_oc, shape_oc, hparams, next_batch, **cfg)
        run.restore(d)
        return run

    def restore(self, d):
        """The non-network part of a checkpoint, in place (also into a run whose step is already recorded).  Lines of
        out_dir/train_log.csv for epochs the checkpoint has not seen (a run killed after an epoch's line and before its checkpoint)
        are dropped: the resumed run writes them again."""
        if d.get("clahe") != self.clahe_record:
            raise ValueError("the checkpoint was written under the CLAHE preprocessing %r and this run's feed has %r: continue with "
                             "the same FundusBatches(clahe=...)" % (d.get("clahe"), self.clahe_record))
        self.train_step.load_state_dict(d["train_step"])
        self.epoch, self.iteration = int(d["epoch"]), int(d["iteration"])
        self._set_term_weights()            # the schedules' values for the epoch that runs next (train_epoch() sets them again)
        if self.validator is not None:
            self.validator.best_mean_dice, self.validator.best_epoch = float(d["best_mean_dice"]), int(d["best_epoch"])
        self.py_rng.setstate(_py_state_from_lists(d["py_rng"]))
        self.np_rng.set_state(_np_state_from_lists(d["np_rng"]))
        self.best = [float(v) for v in d["best"]]
        if d["feed"]:
            if not hasattr(self.next_batch, "load_state"):
                raise ValueError("the checkpoint carries the state of its batch feed (%s) and this run's next_batch cannot take it"
                                 % sorted(d["feed"]))
            self.next_batch.load_state(d["feed"])
        if d.get("swad_state"):
            if self.swad is None:
                raise ValueError("the checkpoint carries the state of its weight averaging (swad) and this run does not average: "
                                 "construct it with swad=")
            self.average.load_state(d["swad_state"]["average"])
            self.swad.load_state(d["swad_state"]["valley"], device=self.log.acc.device)
        path = os.path.join(self.out_dir, "train_log.csv") if self.out_dir is not None else None
        if path is not None and os.path.isfile(path):
            with open(path, newline="") as f:
                rows = list(csv.reader(f))
            keep = rows[:1] + [r for r in rows[1:] if int(r[0]) < self.epoch]
            if len(keep) != len(rows):
                tmp = "%s.tmp%d" % (path, os.getpid())
                with open(tmp, "w", newline="") as f:
                    csv.writer(f).writerows(keep)
                os.replace(tmp, path)
        if d["loss_sums"]:
            self.last = {"epoch": self.epoch - 1, "sums": dict(d["loss_sums"]),
                         "means": {k: v / self.iter_per_epoch for k, v in d["loss_sums"].items()}, "lr": self.train_step.get_lr(), "seconds": 0.0}
