"""The training step: counterpart of the body of the reference's hot loop (Trainer.py:766-914).

One `TrainStep.step()` = the four `update()` calls A-D, their four backward passes and four Adam steps over the
four networks of train.py:91-138, in the reference's order:

    A  seg-net OD   : BCELoss(sigmoid(out), target_od) + gm_i*ins + gm_d*dom            (Trainer.py:779-805)
    B  shape-net OD : kd + gm_i*ins_total + gm_d*dom                                     (:810-825)
       ROI          : od_pred = sigmoid(out) > 0.75 ; roi = (image+1)*od_pred - 1       (:842-853)
    C  seg-net OC   : BCEWithLogits(out*od_pred, target_oc, pos_weight) + wt terms       (:856-892)
    D  shape-net OC : as B on the ROI                                                    (:894-914)

Differences from the reference loop that cannot change a result: no per-iteration `.item()` host syncs or
tensorboard scalars (losses stay on the device), fused Adam over the flat parameter buffer instead of ~390
per-tensor updates, and the dead work listed in shape_networks.py's header is skipped.

Replaying a recorded step: a step is ~1 900 kernel launches from one Python thread (tens of milliseconds of host time,
about as long as the GPU needs for them).  The C ABI allocates nothing, never synchronises and takes nothing that changes
from step to step by value (Adam's step number, its learning rate and the Philox stream position live in device memory), so a step can be
recorded once and replayed:
  * `TrainStep(..., graph="plan")`: the step is recorded under stream capture — which pins every device address: the
    allocator serves the capture from a private pool and defers cross-stream frees — into native launch plans
    (csrc/plan.hip: entry point + argument values + stream of every call, plus the cross-stream waits) and replayed with one
    host call per plan; the captured HIP graph itself is only kept alive as the owner of the memory pool.
  * `TrainStep(..., graph=True)`: the captured HIP graphs themselves are replayed (hipGraphLaunch).  Measured slower than
    eager launches on this runtime (profiles/r02_hipgraph_vs_eager.txt); kept for comparison.
With data-parallel training the gradient all-reduces stay outside (RCCL runs them eagerly between the replayed stretches):
a step is then five plans / graphs with four collectives between them.

What a recording freezes, and what it does not: the learning rates are device floats (`FlatAdam.lr`, `TrainStep.set_lr`: a
stream-ordered write, picked up by the next replay); the optimiser state and the Philox positions are loaded INTO the buffers the
recording reads (`load_state_dict`); betas, eps and the Philox seeds are passed by value and belong to the recording.
"""
import torch

from . import ops
from .boundary import BoundaryLoss
from .lovasz import LovaszLoss
from .overlap import OverlapLoss
from .terms import LossTerm


NET_KEYS = ("od", "od_shape", "oc", "oc_shape")      # the four networks in the order of train.py:120-138 (lr, lr_shape, lr_oc, lr_oc_shape)


def _issue_boundary(term, out, target, mask, dx):
    return ops.boundary_loss(out, ops.signed_distance(target.contiguous()), term.dev, mask=mask, dx=dx)


def _issue_overlap(term, out, target, mask, dx):
    return ops.overlap_loss(out, target.contiguous(), term.dev, term.schedule, mask=mask, dx=dx)


def _issue_lovasz(term, out, target, mask, dx):
    return ops.lovasz_loss(out, target.contiguous(), term.dev, mask=mask, dx=dx)


# The extra terms of calls A and C, in the order they are issued and named: (constructor keyword = stem of the state key, log tag,
# schedule class, issue function (LossTerm.issue)).  TrainStep and TrainRun take everything about a term from here.
TERMS = (("boundary", "bd", BoundaryLoss, _issue_boundary),
         ("overlap", "ov", OverlapLoss, _issue_overlap),
         ("lovasz", "lv", LovaszLoss, _issue_lovasz))


def adam_state_to_torch(m, v, t, shapes, lr, betas, eps):
    """The flat moments m / v (1-D, parameters back to back in `shapes` order) and the step count t as torch.optim.Adam's
    state_dict: state[i] = {step, exp_avg, exp_avg_sq} per parameter, one param_groups entry.  The tensors are copies."""
    state, off = {}, 0
    for i, shape in enumerate(shapes):
        n = 1
        for d in shape:
            n *= int(d)
        state[i] = {"step": torch.tensor(float(t)), "exp_avg": m[off:off + n].reshape(shape).clone(),
                    "exp_avg_sq": v[off:off + n].reshape(shape).clone()}
        off += n
    if off != m.numel() or off != v.numel():
        raise ValueError("the shapes describe %d elements, the moments hold %d / %d" % (off, m.numel(), v.numel()))
    group = {"lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps), "weight_decay": 0, "amsgrad": False,
             "params": list(range(len(shapes)))}
    return {"state": state, "param_groups": [group]}


def adam_state_from_torch(sd, shapes, m, v):
    """The reverse: copies exp_avg / exp_avg_sq of a torch.optim.Adam state_dict into the existing flat m / v (in place) and
    returns (t, param_group).  An empty state (an optimiser that has not stepped) is t = 0 with zero moments; a parameter
    without an entry (torch keeps none for a parameter that never had a gradient) gets zero moments.  One flat step count
    serves all parameters, so a state whose parameters have stepped different numbers of times is refused."""
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError("FlatAdam holds one parameter group (one learning rate per network), the state has %d" % len(groups))
    g = groups[0]
    if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
        raise ValueError("FlatAdam is torch.optim.Adam with weight_decay=0, amsgrad=False, maximize=False; the state asks for "
                         "weight_decay=%r amsgrad=%r maximize=%r" % (g.get("weight_decay"), g.get("amsgrad"), g.get("maximize")))
    if list(g["params"]) != list(range(len(shapes))):
        raise ValueError("the state's parameter group lists %d parameters, the network has %d" % (len(g["params"]), len(shapes)))
    state = sd["state"]
    if len(state) == 0:
        m.zero_()
        v.zero_()
        return 0, g
    # torch.optim.Adam keeps no entry for a parameter that never received a gradient (it skips `p.grad is None`); under a flat
    # update such a parameter sees zero gradients, i.e. zero moments at any step count: that is what a missing entry becomes
    have = [i for i in range(len(shapes)) if i in state]
    steps = sorted({int(float(state[i]["step"])) for i in have})
    if len(steps) != 1:
        raise ValueError("the parameters' step counts differ (%s): one flat step count cannot represent them" % steps)
    for i in have:
        for k in ("exp_avg", "exp_avg_sq"):
            if tuple(state[i][k].shape) != tuple(shapes[i]):
                raise ValueError("parameter %d: %s has shape %s, the network's is %s" % (i, k, tuple(state[i][k].shape), tuple(shapes[i])))
    off = 0
    with torch.no_grad():
        for i, shape in enumerate(shapes):
            n = 1
            for d in shape:
                n *= int(d)
            if i in state:
                m[off:off + n].copy_(state[i]["exp_avg"].reshape(-1))
                v[off:off + n].copy_(state[i]["exp_avg_sq"].reshape(-1))
            else:
                m[off:off + n].zero_()
                v[off:off + n].zero_()
            off += n
    return steps[0], g


class FlatAdam:
    """torch.optim.Adam(lr, betas, eps=1e-8, weight_decay=0) over a network's flat buffers: one launch per step.
    The step count is a device integer and the learning rate a device float (see wtpse_adam_dev in include/wtpse_hip.h): `lr` can
    be assigned at any time, also between the replays of a recorded step — a write on the current stream, no host sync.
    `hold`: optional device int32 (a LossLog's flag); while it is non-zero the launches change neither p nor m nor v."""

    def __init__(self, net, lr=5e-4, betas=(0.9, 0.99), eps=1e-8):
        self.net, self._lr, self.betas, self.eps = net, float(lr), betas, eps
        self.m = self.v = self.t_dev = self.lr_dev = None
        self.hold = None

    def ready(self):
        if self.m is None:
            p = self.net.flat_params()
            self.m = ops.zero_(torch.empty_like(p))
            self.v = ops.zero_(torch.empty_like(p))
            self.t_dev = torch.zeros(1, dtype=torch.int32, device=p.device)      # completed steps
            self.lr_dev = torch.full((1,), self._lr, dtype=torch.float32, device=p.device)

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._lr = float(value)
        if self.lr_dev is not None:
            self.lr_dev.fill_(self._lr)          # rounds to fp32 as the (float) cast of wtpse_adam's by-value lr does

    def step(self):
        net = self.net
        p, g = net.flat_params(), net.flat_grads()
        self.ready()
        ops.adam_step_dev(p, g, self.m, self.v, self.lr_dev, self.betas[0], self.betas[1], self.eps, 1, self.t_dev, self.hold)
        ops.counter_add(self.t_dev, 1)
        net.invalidate_packed()
        net.ensure_ready()

    @property
    def t(self):
        return 0 if self.t_dev is None else int(self.t_dev.item())

    def _shapes(self):
        self.net.ensure_ready()
        return [tuple(p.shape) for p in self.net._plist]      # net.parameters() order = the order of the flat buffer

    def state_dict(self):
        """torch.optim.Adam's layout (adam_state_to_torch), on the device of the network; synchronises (reads the step count)."""
        self.ready()
        return adam_state_to_torch(self.m, self.v, self.t, self._shapes(), self._lr, self.betas, self.eps)

    def load_state_dict(self, sd):
        """From a FlatAdam or a torch.optim.Adam over the same parameters.  Copies into the existing m, v, step count and learning
        rate float: a step that has already been recorded stays valid.  betas / eps are passed to the kernel by value (frozen into
        a recording), so a state with other values than this optimiser's is refused."""
        self.ready()
        g = sd["param_groups"][0] if sd.get("param_groups") else {}
        for k, mine in (("betas", tuple(float(b) for b in self.betas)), ("eps", float(self.eps))):
            theirs = g.get(k, mine)
            theirs = tuple(float(b) for b in theirs) if k == "betas" else float(theirs)
            if theirs != mine:
                raise ValueError("the state was written with %s=%r, this optimiser has %r (passed by value, part of a recorded "
                                 "step): construct the TrainStep with the state's value" % (k, theirs, mine))
        t, g = adam_state_from_torch(sd, self._shapes(), self.m, self.v)
        self.t_dev.fill_(int(t))
        self.lr = g["lr"]


class TrainStep:
    """lr: one rate for all four networks or the 4-tuple (od, od_shape, oc, oc_shape) of train.py:120-138.
    log: optional loss log (wtpse_hip.trainer.LossLog over `TrainStep.log_names(hparams)`).  With one, every call A-D folds its
    loss scalars into the log's device sums with one single-wave launch (wtpse_loss_log) as soon as they exist, calls A and C
    evaluate the reference's NaN test (Trainer.py:794-800, 878-885), and every Adam launch takes the log's flag as `hold`: from the
    first NaN iteration on no parameter and no Adam moment changes any more (the reference raises before backward(); here the
    step never synchronises, so the flag is read by whoever reads the log).  BatchNorm running statistics, the step counts and
    the Philox positions still advance.  With multi-turn > 1 a shape call logs its last turn only (Trainer.py:827-832).
    Without a log (the default) not one extra launch is issued.
    freeze_bn: train on FROZEN BatchNorm statistics — the four networks are kept in eval mode (which changes nothing but BatchNorm:
    update() samples as in training either way), every BatchNorm normalises with its running statistics, which are never written,
    and the backward runs the frozen folds (wtpse_hip/nn.py: _bn_bwd): fine-tuning a trained checkpoint on a few images.  The mode
    is part of a recorded step; step() refuses to run when a network's mode is not the one the step was built for.  It is an
    argument of its own: hparams['freeze_bn'] (which the reference ships and never reads) is NOT looked at.
    average: optional `averaging.WeightAverage` over the networks this step trains, in NET_KEYS order (two when
    hparams['whitening'] is false).  The schedule then ends with ONE more call behind the last Adam launch (wtpse_avg_step: every
    network's new parameters folded into the running means; held by the log's flag like Adam), which lands in the last recorded
    stretch.  Averaging observes and never perturbs: parameters, moments and buffers are those of a step without it.  Without one
    (the default) nothing is issued.
    Extra terms of calls A and C (the table TERMS; each off by default, and then not one launch, buffer or name is added): a term that
    is on makes the objective of the two calls L_seg + w * L_term.  Each call issues its terms in the table's order behind the region
    loss's gradient, in the call's own chain, so they are part of a recorded step: a term yields its unweighted value (`<tag>_od` /
    `<tag>_oc` of the result and of the log, behind the call's other scalars and part of its NaN test) and adds w's share into the
    gradient of the logits.  w is a device float (`set_<term>_weight`: a stream-ordered write that the next replay picks up, like the
    learning rates) that starts at the schedule's weight_at(0); state_dict() carries it as `<term>_weight`.
    boundary: a `boundary.BoundaryLoss`, tag `bd`: L_B = mean(sigmoid(logit) * phi) with phi the signed distance map of the call's
    target (wtpse_signed_distance, then ONE wtpse_boundary_loss; the cup call on the ROI-masked logits, as its region loss).
    overlap: an `overlap.OverlapLoss`, tag `ov`: the soft Dice / Tversky / focal Tversky loss per image of the call's logits against its
    target (ONE wtpse_overlap_loss; the cup call inside the ROI mask; wtpse_hip/overlap.py).
    lovasz: a `lovasz.LovaszLoss`, tag `lv`: the Lovász hinge loss per image of the call's logits against its target (ONE
    wtpse_lovasz_loss: a segmented stable sort of every plane on the device; the cup call over the pixels of the ROI mask only;
    wtpse_hip/lovasz.py)."""

    def __init__(self, model_od, shape_od, model_oc, shape_oc, hparams, lr=5e-4, betas=(0.9, 0.99), dp=None, graph=False, log=None,
                 freeze_bn=False, average=None, boundary=None, overlap=None, lovasz=None):
        self.hp = hparams
        self.freeze_bn = bool(freeze_bn)
        if self.freeze_bn and dp is not None:
            raise ValueError("freeze_bn=True is not supported together with data-parallel training (dp=)")
        if average is not None and dp is not None:
            raise ValueError("average= is not supported together with data-parallel training (dp=)")
        given = dict(boundary=boundary, overlap=overlap, lovasz=lovasz)
        self.terms = []                 # the terms that are on, in TERMS' order
        for key, tag, _, issue in TERMS:
            if given[key] is not None:
                if dp is not None:
                    raise ValueError("%s= is not supported together with data-parallel training (dp=)" % key)
                self.terms.append(LossTerm(key, tag, given[key], issue, next(model_od.parameters()).device))
        self.full = bool(hparams['whitening'])
        self.nets = [model_od, model_oc] + ([shape_od, shape_oc] if self.full else [])
        self.model_od, self.shape_od, self.model_oc, self.shape_oc = model_od, shape_od, model_oc, shape_oc
        self.dp = dp
        for n in self.nets:
            n.train(not self.freeze_bn)
            n.ensure_ready(repack=True)
            object.__setattr__(n, "_packed_valid", True)     # this harness owns the optimiser and repacks after each step
            object.__setattr__(n, "_attach_grads", False)
            object.__setattr__(n, "_dp", dp)
            object.__setattr__(n, "_defer_allreduce", True)  # the gradient exchange is issued here, between backward and Adam
        if dp is not None:
            dp.broadcast_params(self.nets)
        lrs = tuple(lr) if isinstance(lr, (tuple, list)) else (lr,) * 4
        if len(lrs) != 4:
            raise ValueError("lr: one rate or the four (od, od_shape, oc, oc_shape), got %d values" % len(lrs))
        self.by_key = {k: n for k, n in zip(NET_KEYS, (model_od, shape_od, model_oc, shape_oc)) if any(n is x for x in self.nets)}
        # (keyed by network, looked up by id() everywhere: its order — NET_KEYS', not self.nets' — carries no meaning)
        self.opt = {id(self.by_key[k]): FlatAdam(self.by_key[k], r, betas) for k, r in zip(NET_KEYS, lrs) if k in self.by_key}
        self.average = average
        if average is not None:
            trained = [self.by_key[k] for k in NET_KEYS if k in self.by_key]
            if len(average.nets) != len(trained) or any(a is not b for a, b in zip(average.nets, trained)):
                raise ValueError("average= must be a WeightAverage over the %d networks this step trains, in the order %s"
                                 % (len(trained), [k for k in NET_KEYS if k in self.by_key]))
        self.log = log
        if log is not None:
            want = self.log_names(hparams, **{t.key: True for t in self.terms})
            if list(log.names) != want:
                raise ValueError("the loss log's names must be TrainStep.log_names(hparams%s) = %s, got %s"
                                 % ("".join(", %s=True" % t.key for t in self.terms), want, list(log.names)))
        for o in self.opt.values():
            o.ready()
            o.hold = None if log is None else log.flag
        self.last_od_pred = None
        # exact data-parallel mode runs ~100 small collectives inside every forward: it stays eager
        self.graph = bool(graph) and not (dp is not None and dp.exact)
        self.plan = self.graph and graph == "plan"
        self._graphs = None
        self._static = None

    # ------------------------------------------------------------------------------------------------ schedule
    def _seg_call(self, model, x, target, noise, od_pred):
        """forward + loss + backward of one segmentation network, then (after the caller's gradient exchange) Adam.
        Generator: yields the network whose flat gradient is ready to be exchanged; returns (logits, losses)."""
        gi, gd = float(self.hp['instance_wt_gm']), float(self.hp['domain_wt_gm'])
        if noise is not None:
            model.set_noise([noise])
        res, tape = model._forward_update(x, target, x, want_tape=True)
        out = res[0]
        if od_pred is None:
            loss = ops.bce_sigmoid_fwd(out, target)
            d_out = ops.bce_sigmoid_bwd(out, target)
        else:
            sums, pw = ops.pos_weight_sums(od_pred, target)
            if self.dp is not None and self.dp.exact:      # pos_weight over the global batch (Trainer.py:865)
                pw = ops.pos_weight_from_sums(self.dp.allreduce_sum(sums))
            loss = ops.bce_logits_pw_fwd(out, od_pred, target, pw)
            d_out = ops.bce_logits_pw_bwd(out, od_pred, target, pw)
        r = {"seg": loss}
        if self.full:
            r["ins"], r["dom"] = res[2][0], res[2][3]
        for t in self.terms:            # w * L_term on top: its gradient joins the region loss's, its value the call's NaN test
            r[t.tag] = t.issue(out, target, od_pred, d_out)
        # the reference's running sums and NaN test of this call (Trainer.py:788-800 / 874-885), in front of backward and Adam: every
        # scalar of the call is tested
        self._log("seg_od" if od_pred is None else "seg_oc", list(r.values()), ops.loss_log_code(len(r)), model)
        model._backward_update(tape, d_out, None, None, w_ins=gi, w_dom=gd)
        del tape
        yield model
        self.opt[id(model)].step()
        return out, r

    def _shape_call(self, shape, model, x, target):
        gi, gd = float(self.hp['instance_wt_gm']), float(self.hp['domain_wt_gm'])
        r = None
        turns = int(self.hp['multi-turn'])
        for turn in range(turns):
            scal, tape = shape._forward_update(model, x, target, want_tape=True)
            if turn == turns - 1:       # the last turn's values only (Trainer.py:827-832, 915-919); the shape losses are never NaN-tested
                od = shape is self.shape_od
                self._log("kd_od" if od else "kd_oc", [scal[0], scal[1], scal[2], scal[3], scal[4]] if od else [scal[0], scal[1], scal[4]],
                          0, shape)
            shape._backward_update(tape, None, None, None, None, w_kd=1.0, w_off=gi, w_diag=gi, w_dom=gd)
            del tape
            yield shape
            self.opt[id(shape)].step()
            r = {"kd": scal[0], "ins_total": scal[1], "ins_off": scal[2], "ins_diag": scal[3], "dom": scal[4]}
        return r

    def _schedule(self, image, target_od, target_oc, noise):
        """The step as a generator that yields at the points where a network's gradient is complete and not yet used."""
        out, ra = yield from self._seg_call(self.model_od, image, target_od, noise.get("a"), None)
        res = self._call_names(ra, "od")
        if self.full:
            rb = yield from self._shape_call(self.shape_od, self.model_od, image, target_od)
            res.update(kd_od=rb["kd"], ins_shape_od=rb["ins_total"], ins_ij_od=rb["ins_off"], ins_ii_od=rb["ins_diag"],
                       dom_shape_od=rb["dom"])
        roi, od_pred = ops.roi(image, out)
        self.last_od_pred = od_pred          # [B,1,H,W] in {0,1}: lets a caller see how much of the image the ROI keeps
        out_oc, rc = yield from self._seg_call(self.model_oc, roi, target_oc, noise.get("c"), od_pred)
        res.update(self._call_names(rc, "oc"))
        if self.full:
            rd = yield from self._shape_call(self.shape_oc, self.model_oc, roi, target_oc)
            res.update(kd_oc=rd["kd"], ins_shape_oc=rd["ins_total"], dom_shape_oc=rd["dom"])
        if self.average is not None:     # behind the last Adam launch: the iterate this step has produced, all networks in one call
            self.average.update(hold=self.log.flag if self.log is not None else None)
        return res

    @staticmethod
    def _call_names(r, call):
        """A segmentation call's scalars {tag: value} under their names in the result and in the log: tag + "_od" / tag + "_oc"."""
        return {tag + "_" + call: v for tag, v in r.items()}

    @staticmethod
    def log_names(hparams, boundary=False, overlap=False, lovasz=False):
        """The loss names in the order a LossLog for this step holds them: the keys of step()'s result, call by call (A-D).
        boundary, overlap, lovasz: with the term's `bd_*` / `ov_*` / `lv_*`; the terms that are on follow the other names of their call (A / C) in TERMS'
        order, so that the call's one wtpse_loss_log launch covers them."""
        full = bool(hparams['whitening'])
        given = dict(boundary=boundary, overlap=overlap, lovasz=lovasz)
        tags = (["seg", "ins", "dom"] if full else ["seg"]) + [tag for key, tag, _, _ in TERMS if given[key]]
        shape = {"od": ["kd_od", "ins_shape_od", "ins_ij_od", "ins_ii_od", "dom_shape_od"], "oc": ["kd_oc", "ins_shape_oc", "dom_shape_oc"]}
        names = []
        for call in ("od", "oc"):
            names += [tag + "_" + call for tag in tags] + (shape[call] if full else [])
        return names

    def _log(self, first, scalars, check_n, net):
        """One wtpse_loss_log launch: `scalars` into the log's slots that start at name `first`."""
        if self.log is not None:
            ops.loss_log(scalars, self.log.acc, self.log.names.index(first), check_n, self.log.flag, self.opt[id(net)].t_dev)

    def _exchange(self, net):
        if self.dp is not None:
            self.dp.allreduce_grads(net, net.flat_grads())

    # ------------------------------------------------------------------------------------------------ hipGraph
    def _capture(self, image, target_od, target_oc):
        """Record the step into HIP graphs / launch plans (one per stretch between gradient exchanges).  Nothing executes
        while a stretch is recorded; the eager collectives between two stretches run on stale buffers and are harmless."""
        self._static = tuple(t.clone() for t in (image, target_od, target_oc))
        pool = torch.cuda.graph_pool_handle()
        self._cap_stream = torch.cuda.Stream(device=image.device)
        gen = self._schedule(*self._static, {})
        graphs, res = [], None
        L = ops.lib()
        done = False
        # the recorded launches' ticket slices: a buffer of the recording's own, never the eager ring (ops.ticket_scope)
        self._ticket_scope = ops.ticket_scope(image.device)
        with self._ticket_scope:
            self._capture_stretches(gen, pool, L, graphs)
        res = self._capture_result
        self._graphs, self._result = graphs, res

    def _capture_stretches(self, gen, pool, L, graphs):
        res, done = None, False
        while not done:
            g = torch.cuda.CUDAGraph()
            net = plan = None
            if self.plan:
                L.plan_begin()
            try:
                # thread_local: another thread's HIP calls (the RCCL watchdog polling the events of the parameter broadcast that
                # ran before the capture) must not invalidate the capture — in "global" mode they did, now and then (status 901)
                with torch.cuda.graph(g, pool=pool, stream=self._cap_stream, capture_error_mode="thread_local"):
                    try:
                        net = next(gen)
                    except StopIteration as stop:
                        res, done = stop.value, True
                    except BaseException:
                        # leaving a broken capture can crash the runtime before Python reports anything: say why first
                        import traceback
                        traceback.print_exc()
                        raise
            finally:
                if self.plan:
                    plan = L.plan_end()
            graphs.append((g, net, plan))
            if net is not None:
                self._exchange(net)
        self._capture_result = res

    def _replay(self):
        L = ops.lib()
        for g, net, plan in self._graphs:
            if plan is not None:
                cur = torch.cuda.current_stream()
                self._cap_stream.wait_stream(cur)       # the plan's streams start behind the caller's stream ...
                try:
                    L.plan_replay(plan)
                except Exception:
                    # a recorded call failed mid-plan: the side streams forked inside the plan were never joined, so nothing
                    # may run unordered behind them — drain the device before the error propagates
                    torch.cuda.synchronize()
                    raise
                finally:
                    cur.wait_stream(self._cap_stream)   # ... and the caller's stream continues behind the plan
            else:
                g.replay()
            if net is not None:
                self._exchange(net)

    # ------------------------------------------------------------------------------------------------ rates and state
    def set_lr(self, od=None, od_shape=None, oc=None, oc_shape=None):
        """New learning rates (None: unchanged) from the next step on, recorded or not: stream-ordered writes, no host sync."""
        for k, r in zip(NET_KEYS, (od, od_shape, oc, oc_shape)):
            if r is not None and k in self.by_key:
                self.opt[id(self.by_key[k])].lr = r

    def get_lr(self):
        """{network key: rate} as last set (host values)."""
        return {k: self.opt[id(n)].lr for k, n in self.by_key.items()}

    def _term(self, key, attr):
        """An attribute of the term `key`; None when the term is off."""
        return next((getattr(t, attr) for t in self.terms if t.key == key), None)

    def set_term_weight(self, key, w):
        """The weight of the term `key` from the next step on, recorded or not: a stream-ordered write of the device float the kernel
        reads (rounded to fp32), no host sync."""
        set_weight = self._term(key, "set_weight")
        if set_weight is None:
            raise ValueError("this TrainStep has no %s term (TrainStep(%s=...))" % (key, key))
        set_weight(w)

    def get_term_weight(self, key):
        """The weight as last set (the host value; None when the term is off)."""
        return self._term(key, "weight")

    # the terms under their public names: the schedule object, the device weight, the weight's setter and getter
    boundary = property(lambda self: self._term("boundary", "schedule"))
    overlap = property(lambda self: self._term("overlap", "schedule"))
    bd_alpha = property(lambda self: self._term("boundary", "dev"))
    ov_w = property(lambda self: self._term("overlap", "dev"))
    lovasz = property(lambda self: self._term("lovasz", "schedule"))
    lv_w = property(lambda self: self._term("lovasz", "dev"))

    def set_boundary_weight(self, a):
        self.set_term_weight("boundary", a)

    def get_boundary_weight(self):
        return self.get_term_weight("boundary")

    def set_overlap_weight(self, w):
        self.set_term_weight("overlap", w)

    def get_overlap_weight(self):
        return self.get_term_weight("overlap")

    def set_lovasz_weight(self, w):
        self.set_term_weight("lovasz", w)

    def get_lovasz_weight(self):
        return self.get_term_weight("lovasz")

    def state_dict(self):
        """What a run needs beside the networks' own state_dict()s to continue where it stopped: per network the optimiser state
        (torch.optim.Adam's layout, FlatAdam.state_dict) and the Philox seed and position of its sampling noise; per term that is on
        its current weight.  Synchronises."""
        sd = {"optim": {k: self.opt[id(n)].state_dict() for k, n in self.by_key.items()},
              "noise": {k: {"seed": int(n._noise_seed), "ctr": int(n._noise_ctr.item())} for k, n in self.by_key.items()}}
        sd.update({t.key + "_weight": float(t.weight) for t in self.terms})
        return sd

    def load_state_dict(self, sd):
        """Restores everything in place (moments, step counts, learning rates, Philox positions), so a step that has already been
        recorded stays valid and continues from the loaded state.  The Philox SEED is passed to the kernels by value and is frozen
        into a recording: once this TrainStep holds one, a state with another seed is refused.  Load the networks' own
        state_dict()s first: their packed weight copies are refreshed here (a replayed step does not look at them again)."""
        if set(sd["optim"]) != set(self.by_key) or set(sd["noise"]) != set(self.by_key):
            raise ValueError("the state holds the networks %s, this step trains %s" % (sorted(sd["optim"]), sorted(self.by_key)))
        for k, n in self.by_key.items():
            seed = int(sd["noise"][k]["seed"])
            if seed != int(n._noise_seed) and self._graphs is not None:
                raise ValueError("network %r: the state's Philox seed %d differs from the seed %d this TrainStep has recorded (the seed "
                                 "is passed by value): seed the networks with seed_noise(%d) before the first step, or close() and "
                                 "record again" % (k, seed, n._noise_seed, seed))
        for k, n in self.by_key.items():
            self.opt[id(n)].load_state_dict(sd["optim"][k])
            n.ensure_ready()
            object.__setattr__(n, "_noise_seed", int(sd["noise"][k]["seed"]))
            n._noise_ctr.fill_(int(sd["noise"][k]["ctr"]))
        for t in self.terms:
            if t.key + "_weight" in sd:         # (a state from before the term: the weight stays)
                t.set_weight(sd[t.key + "_weight"])

    def close(self):
        """Release the native launch plans (and their hipEvents) of a recorded step."""
        graphs, self._graphs = self._graphs, None
        if graphs:
            L = ops.lib()
            for _, _, plan in graphs:
                if plan is not None:
                    L.plan_destroy(plan)
            self._ticket_scope = None       # the recorded launches' ticket buffer goes with them

    def __del__(self):
        import sys
        if sys.is_finalizing():       # the HIP runtime may already be gone: destroying events then aborts the process
            return
        try:
            self.close()
        except Exception:
            pass

    def step(self, image, target_od, target_oc, noise=None):
        """image [B,3,H,W] in [-1,1], targets [B,1,H,W] in {0,1}; all device fp32, rows domain-major.
        noise: optional {'a': eps, 'c': eps} standard-normal [B,1,H,W] (parity runs); default Philox.
        Returns {name: 0-dim device tensor}; nothing is synchronised with the host.  With graph=True the returned tensors
        are the graphs' own output buffers: read them before the next step() overwrites them."""
        image = image.contiguous()
        for n in self.nets:
            if any(m.training == self.freeze_bn for m in n.modules()):
                raise RuntimeError("this TrainStep was built with freeze_bn=%r: its networks must be in %s mode (the schedule — and a "
                                   "recorded step — belongs to that mode); a module of %s is not"
                                   % (self.freeze_bn, "eval" if self.freeze_bn else "train", type(n).__name__))
        if self.graph and not noise:
            if self._graphs is None:
                self._capture(image, target_od, target_oc)
            for dst, src in zip(self._static, (image, target_od, target_oc)):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src)
            if self.average is not None:
                self.average.tick()         # the recorded update() executes once per replay
            self._replay()
            return self._result
        gen = self._schedule(image, target_od, target_oc, noise or {})
        try:
            while True:
                self._exchange(next(gen))
        except StopIteration as stop:
            return stop.value
