"""Thin host wrappers over the C ABI (include/wtpse_hip.h): allocate outputs/scratch with torch (device
memory + stream plumbing only) and launch on torch's current HIP stream.  No arithmetic happens here."""
import torch

from .lib import lib

_WS = {}


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr():
    """Raw hipStream_t of torch's current stream (the C getter: torch.cuda.current_stream() builds a Python Stream object
    on every call, ~8 us, and this runs once per launch)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, name="tensor"):
    if t is None:
        return
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous fp32 tensor in device memory (got %s, %s, contiguous=%s)"
                         % (name, t.device, t.dtype, t.is_contiguous()))


def workspace(tag, nfloats, device):
    """Persistent scratch, one buffer per (device, stream, tag), grown on demand: independent parts of the schedule run on
    different streams (nn.py) and must not share scratch."""
    key = (str(device), stream_ptr(), tag)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(int(nfloats), 1024), dtype=torch.float32, device=device)
        _WS[key] = buf
    return buf


# ----------------------------------------------------------------------------------------------- convolution
def _out_pair(split, B, cout, H, W, device):
    """-> (out0, out1 or None, csplit): the output of a launch, in two tensors cut at channel `split` when one is given."""
    if split is None:
        return torch.empty((B, cout, H, W), dtype=torch.float32, device=device), None, cout
    csplit = int(split)
    return (torch.empty((B, csplit, H, W), dtype=torch.float32, device=device),
            torch.empty((B, cout - csplit, H, W), dtype=torch.float32, device=device), csplit)


def _stats_blocks(layout, B, H, W, cout=0, ksize=0):
    """Rows of the per-workgroup partials of a launch on the packed layout `layout` (0 fp32, 1 x3, 2 the 16-channel x3 fragments)."""
    if layout == 1:
        return lib().query("wtpse_conv_x3_stats_blocks", B, H, W, cout, int(ksize))
    return lib().query("wtpse_conv_stats_blocks", B, H, W)


def _conv_launch(name, layout, in_amax, in0, in1, wpacked_ptr, bias, cout, ksize, pro0, pro_relu, relu_out, want_stats, split, mask_ref,
                 pro1, out_amax):
    """conv_fwd / conv_fwd_x3: entry point `name`; in_amax: the pointers wtpse_conv_fwd_x3 takes in front of out_amax."""
    _chk(in0, "in0"); _chk(in1, "in1"); _chk(pro0, "pro0"); _chk(pro1, "pro1")
    B, C0, H, W = in0.shape
    C1 = 0 if in1 is None else in1.shape[1]
    out0, out1, csplit = _out_pair(split, B, cout, H, W, in0.device)
    stats = None
    if want_stats:
        stats = torch.empty((_stats_blocks(layout, B, H, W, cout, ksize), cout, 2), dtype=torch.float32, device=in0.device)
    lib().call(name, ptr(in0), C0, ptr(in1), C1, wpacked_ptr, ptr(bias), ptr(pro0), ptr(pro1), int(pro_relu), ptr(out0),
               ptr(out1), csplit, ptr(stats), B, H, W, cout, ksize, int(relu_out), ptr(mask_ref), *in_amax, ptr(out_amax), stream_ptr())
    if out_amax is not None:
        amax_attach(out0, out_amax)
    return out0, out1, stats


def conv_fwd(in0, in1, wpacked_ptr, bias, cout, ksize, pro0=None, pro_relu=0, relu_out=False, want_stats=False,
             split=None, mask_ref=None, pro1=None, out_amax=None):
    """-> (out0, out1 or None, stats or None).  `wpacked_ptr` is a raw device pointer into the packed-weight buffer.
    out_amax: a zeroed amax table (fwd_amax_table) that receives the largest magnitude of the stored output."""
    return _conv_launch("wtpse_conv_fwd", 0, (), in0, in1, wpacked_ptr, bias, cout, ksize, pro0, pro_relu, relu_out, want_stats, split,
                        mask_ref, pro1, out_amax)


def conv_fwd_gram(in0, wpacked_ptr, bias, pro0=None, pro_relu=0, relu_out=False, out_amax=None):
    """3x3 conv with 16 output channels that also returns the per-tile partial Grams of its output.
    -> (out, (partial [B*S,256], S)) with S = tiles per image: what wt_loss_fwd(..., gram_partial=) takes."""
    _chk(in0, "in0"); _chk(pro0, "pro0")
    B, C0, H, W = in0.shape
    L = lib()
    out = torch.empty((B, 16, H, W), dtype=torch.float32, device=in0.device)
    nblk = _stats_blocks(0, B, H, W)
    partial = torch.empty((nblk, 256), dtype=torch.float32, device=in0.device)
    L.call("wtpse_conv_fwd_gram", ptr(in0), C0, wpacked_ptr, ptr(bias), ptr(pro0), int(pro_relu), ptr(out), ptr(partial), B, H, W,
           16, int(relu_out), ptr(out_amax), stream_ptr())
    if out_amax is not None:
        amax_attach(out, out_amax)
    return out, (partial, nblk // B)


X16_SIZE = 8 + 5 * 3 * 64 * 8 + 5 * 2 * 64 * 8      # unsigned shorts of one direction of one conv in the 16-channel layout: header, x3 and x2h fragments


def conv16_x3(in0, wx16_ptr, bias, cout, pro0=None, pro_relu=0, relu_out=False, want_stats=False, want_gram=False, mask_ref=None,
              bnb=None, grad_in=False, in_amax=None, out_amax=None):
    """3x3 conv with at most 16 input and 16 output channels in the x3 / x2h arithmetic (csrc/conv.hip MODE 3 / 4; include/wtpse_hip.h,
    wtpse_conv16_x3).  bnb = (bn_y, bn_ss, bn_mean, bn_relu): the BatchNorm-backward epilogue of dgrad_bnb.  grad_in: in0 is a
    gradient (a data-gradient launch): x2h only with the amax table its producer attached (`in0.wt_amax`), x3 otherwise — never an
    extra pass for it.  in_amax (forward launches): the bound of the input as loaded; out_amax: as conv_fwd.
    -> (out, stats or None, (gram partial, tiles per image) or None)."""
    _chk(in0, "in0"); _chk(pro0, "pro0"); _chk(mask_ref, "mask_ref")
    B, C0, H, W = in0.shape
    L = lib()
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=in0.device)
    nblk = _stats_blocks(2, B, H, W)
    stats = torch.empty((nblk, cout, 2), dtype=torch.float32, device=in0.device) if (want_stats or bnb is not None) else None
    gram = torch.empty((nblk, 256), dtype=torch.float32, device=in0.device) if want_gram else None
    bn_ss = bn_mean = None
    bn_relu = 0
    if bnb is not None:
        mask_ref, bn_ss, bn_mean, bn_relu = bnb
        _chk(mask_ref, "bn_y"); _chk(bn_ss, "bn_ss"); _chk(bn_mean, "bn_mean")
        assert mask_ref.shape == out.shape
    L.call("wtpse_conv16_x3", ptr(in0), C0, wx16_ptr, ptr(bias), ptr(pro0), int(pro_relu), ptr(out), ptr(stats), ptr(gram),
           ptr(mask_ref), ptr(bn_ss), ptr(bn_mean), int(bool(bn_relu)), B, H, W, cout, int(relu_out), int(bool(grad_in)),
           ptr(amax_attached(in0)) if grad_in else ptr(in_amax), ptr(out_amax), stream_ptr())
    if out_amax is not None:
        amax_attach(out, out_amax)
    return out, stats, ((gram, nblk // B) if want_gram else None)


def x3_packed_size(rows, k, taps):
    """unsigned shorts of one direction of one conv in the x3 layout (include/wtpse_hip.h): 64 bytes of header + the term slots."""
    return 32 + ((k + 15) & ~15) * ((rows + 31) & ~31) * taps * 3


def x3_terms():
    """16-bit terms per fp32 operand in the x3 kernels right now (wtpse_x3_terms: 3 x3, 2 x2h, 1 bf16 mode)."""
    return lib().query("wtpse_x3_terms", -1)


AMAX_WORDS = 1024           # unsigneds of one amax table (include/wtpse_hip.h, wtpse_amax): 64 shards, one per 64-byte line
_AMAX = {}
_AMAX_TABLES = 512          # tables per arena (2 MB): a backward pass of the largest network hands out ~120


class _Arena:
    """An int32 buffer, zero when it is handed over, given out front to back: `buf` (None: no buffer), `next` = words given out so
    far, take(n_words) -> the next slice, or None when there is no buffer or it is exhausted (the owner decides what happens
    then).  renew(buf) starts over on a fresh buffer and keeps the last three in `retired` for work still queued on them."""
    __slots__ = ("buf", "next", "retired")

    def __init__(self, buf):
        self.buf, self.next, self.retired = buf, 0, []

    def take(self, n):
        off = self.next
        if self.buf is None or off + n > self.buf.numel():
            return None
        self.next = off + n
        return self.buf[off:off + n]

    def renew(self, buf):
        self.retired.append(self.buf)
        del self.retired[:-3]
        self.buf, self.next = buf, 0

    def __getitem__(self, i):       # (buf, next) by position: how the kernel tests have always read the ticket ring
        return (self.buf, self.next)[i]


def amax_begin(device):
    """Start of a backward pass: a fresh arena of zeroed amax tables for the gradients it produces.  ONE launch zeroes the WHOLE arena,
    unconditionally — the call is part of recorded launch plans / captured graphs, so what it zeroes must not depend on how many
    tables the pass before it happened to use when the step was recorded (a conditional, sized zeroing left the replayed steps with
    the tables of earlier steps: scales that only ever grew, results that differed from the eager step in the last bits).
    Round 6: the arena is a buffer of the PASS, not of the device — rounds 5's one arena per device was zeroed wholesale
    by whichever network began a backward pass next, under the feet of a pass of another network still in flight.  The producers of a
    pass (bn_bwd_*, upsample2x_bwd*) take their tables with _amax_table(); the tables (views, attached to the gradients as
    `wt_amax`) keep their arena alive, and the last few arenas are held a little longer for work still queued on side streams."""
    buf = zero_(torch.empty(_AMAX_TABLES * AMAX_WORDS, dtype=torch.int32, device=device))     # (2 MB, ~2 us; recorded steps: from the capture's pool)
    st = _AMAX.get(device)
    if st is None:
        _AMAX[device] = _Arena(buf)
    else:
        st.renew(buf)


def _amax_table(device):
    """A zeroed amax table for a producer, or None when the x2h arithmetic is off (nothing would read it)."""
    if x3_terms() != 2:
        return None
    st = _AMAX.get(device)
    t = st.take(AMAX_WORDS) if st is not None else None
    # no arena yet / exhausted (micro-benchmarks looping without begin_backward): a fresh zeroed table
    return t if t is not None else zero_(torch.empty(AMAX_WORDS, dtype=torch.int32, device=device))


_FWD_SCOPES = []
FWD_SCOPE_TABLES = 256      # per forward pass (1 MB): a WT_PSE.update hands out ~60, an eval-mode predict ~170


class fwd_scope(_Arena):
    """The amax tables of ONE forward pass (an update() / predict() call): forward activations carry a bound of their largest
    magnitude to their x2h consumers in tables like the gradients' (include/wtpse_hip.h, wtpse_x3_terms), and those tables must be zero
    when their producer runs.  A scope owns one buffer, zeroed by ONE launch when the pass starts (on the stream the pass starts on,
    in front of every fork), and hands out slices; the slices (held by the activations on the tape) keep the buffer alive until the
    backward pass is done with them.  Recorded steps: the buffer comes from the capture's pool and the zeroing is a recorded launch.
    Without a scope (block-level callers, tests) a table is a fresh zeroed tensor of its own."""
    __slots__ = ()

    def __init__(self, device):
        super().__init__(zero_(torch.empty(FWD_SCOPE_TABLES * AMAX_WORDS, dtype=torch.int32, device=device)) if x3_terms() == 2 else None)

    def __enter__(self):
        _FWD_SCOPES.append(self)
        return self

    def __exit__(self, *exc):
        assert _FWD_SCOPES and _FWD_SCOPES[-1] is self
        _FWD_SCOPES.pop()
        return False


def fwd_amax_table(device):
    """A zeroed amax table for the producer of a forward activation, or None when the x2h arithmetic is off (nobody would read it)."""
    if x3_terms() != 2:
        return None
    sc = _FWD_SCOPES[-1] if _FWD_SCOPES else None
    t = sc.take(AMAX_WORDS) if sc is not None and sc.buf is not None and sc.buf.device == device else None
    return t if t is not None else zero_(torch.empty(AMAX_WORDS, dtype=torch.int32, device=device))


def act_bound(ss, raw_amax):
    """Amax table of |ss[c,0] * y + ss[c,1]| over a tensor y whose amax table is raw_amax (include/wtpse_hip.h, wtpse_act_bound)."""
    tab = torch.empty(AMAX_WORDS, dtype=torch.int32, device=ss.device)
    lib().call("wtpse_act_bound", ptr(ss), ss.shape[0], ptr(raw_amax), ptr(tab), stream_ptr())
    return tab


def _version(t):
    try:
        return t._version
    except RuntimeError:            # a tensor made under torch.inference_mode() tracks no version: the table stays with the object
        return -1


def amax_attach(t, tab):
    """Attach the amax table `tab` to the tensor t, for the contents t has (or is about to be given by the launch that fills tab):
    the table is valid for as long as t is not written again.  In-place writes through torch move `t._version`, which is kept next
    to the table; the library's own in-place launches (raw pointers: no version) say so with _amax_stale."""
    t.wt_amax = tab
    if tab is not None:
        t.wt_amax_version = _version(t)


def amax_attached(t):
    """The amax table attached to t if it still describes t's contents, else None: a caller who wrote into t in place since
    (x.copy_(batch), dz.mul_(s)) gets a fresh look at the data instead of the scale of the contents before."""
    tab = getattr(t, "wt_amax", None)
    if tab is not None and getattr(t, "wt_amax_version", None) != _version(t):
        t.wt_amax = tab = None
    return tab


def amax_of(t):
    """The amax table (int32 tensor [AMAX_WORDS]) of the tensor t as stored: the scale source of an operand of the x2h kernels.
    Producers that fill it as they write t (bn_bwd_*, upsample2x_bwd*; the convolutions' epilogues for un-normalised forward maps) attach
    it to their result (amax_attach); anything else pays one extra pass here (and keeps the table on the tensor for its other
    consumers, until the tensor is written again: amax_attached)."""
    tab = amax_attached(t)
    if tab is None:
        tab = torch.empty(AMAX_WORDS, dtype=torch.int32, device=t.device)
        lib().call("wtpse_amax", ptr(t), t.numel(), ptr(tab), stream_ptr())
        amax_attach(t, tab)
    return tab


def conv_fwd_x3(in0, in1, wpacked_ptr, bias, cout, ksize, pro0=None, pro_relu=0, relu_out=False, want_stats=False,
                split=None, mask_ref=None, pro1=None, in_amax=None, in_amax1=None, out_amax=None):
    """conv_fwd on the 16-bit matrix cores at fp32 accuracy (csrc/conv_x3.hip); `wpacked_ptr` points into the x3-packed weights.
    in_amax / in_amax1: the amax tables of in0 / in1 AS LOADED (a gradient's amax_of; a forward activation's bound, nn.act_amax) —
    include/wtpse_hip.h, wtpse_x3_terms; out_amax: as conv_fwd."""
    return _conv_launch("wtpse_conv_fwd_x3", 1, (ptr(in_amax), ptr(in_amax1)), in0, in1, wpacked_ptr, bias, cout, ksize, pro0, pro_relu,
                        relu_out, want_stats, split, mask_ref, pro1, out_amax)


_TICKETS = {}               # device -> _Arena: the eager ring
_TICKET_RING = 1 << 22      # unsigneds (16 MB): ~1900 launches of the largest layer (5 training steps) before a slice comes round again; the
                            # streams of a step are joined at its end, so two users of a slice never run at the same time
_TICKET_SCOPE = None        # the ticket_scope a step is being recorded under: its private ticket buffer
_DEBUG = __import__("os").environ.get("WTPSE_DEBUG", "0") == "1"


class ticket_scope(_Arena):
    """While a step is recorded into a launch plan / captured into a graph, its launches take their ticket slices from a buffer of
    their OWN (allocated here, before the capture starts; owned by the recorded step and freed with it) instead of the eager ring:
    a replayed launch keeps its slice for as long as the recording lives, and the eager ring's pointer, which comes round every
    ~1900 launches, must never land on it (an eager step between two replays would have shared slices with the
    replayed launches that were in flight on other streams)."""
    __slots__ = ()

    def __init__(self, device, n=1 << 21):
        super().__init__(torch.zeros(n, dtype=torch.int32, device=device))
        torch.cuda.current_stream(device).synchronize()

    def __enter__(self):
        global _TICKET_SCOPE
        assert _TICKET_SCOPE is None, "ticket scopes do not nest"
        self.next = 0
        _TICKET_SCOPE = self
        return self

    def __exit__(self, *exc):
        global _TICKET_SCOPE
        _TICKET_SCOPE = None
        return False


def _tickets(n, device):
    """n zeroed unsigneds for a launch that leaves them zeroed (include/wtpse_hip.h: wtpse_dgrad_bnb_coef).  Eager launches: slices
    of one ring per device — a slice is handed out again only after ~1900 further launches, long after its launch has finished.
    Launches recorded inside a ticket_scope: consecutive slices of the scope's private buffer, never reused.  -> (pointer, view)."""
    n = (n + 63) & ~63
    st = _TICKET_SCOPE
    if st is not None:
        view = st.take(n)
        if view is None:
            raise RuntimeError("ticket_scope exhausted (%d unsigneds): a recorded step uses more ticket words than reserved" % st.buf.numel())
        return st.buf.data_ptr() + 4 * view.storage_offset(), view
    st = _TICKETS.get(device)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            # the zero fill would be captured instead of executed (and the ring would live in the capture's private pool)
            raise RuntimeError("the ticket ring must exist before a step is captured: HipNet.ensure_ready() creates it")
        st = _TICKETS[device] = _Arena(torch.zeros(_TICKET_RING, dtype=torch.int32, device=device))
        torch.cuda.current_stream(device).synchronize()
    view = st.take(n)
    if view is None:                # the ring comes round
        st.next = 0
        view = st.take(n)
    if _DEBUG and n and not torch.cuda.is_current_stream_capturing():
        torch.cuda.synchronize(device)
        off = view.storage_offset()
        assert not bool(view.any()), "ticket slice [%d, %d) is not zero on entry: a launch that used it failed or is still running" % (off, off + n)
    return st.buf.data_ptr() + 4 * view.storage_offset(), view


def _ticket_call(view, name, *args):
    """lib().call for a launch that owns the ticket slice `view`: a launch that fails (rejected arguments after the slice was
    taken, a launch error) may leave its slice half-counted — it is re-zeroed (after a device sync) before the error propagates,
    so that the launch that gets the slice next does not fold its statistics one arrival early."""
    try:
        lib().call(name, *args)
    except Exception:
        if view.numel() and not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(view.device)
            zero_(view)
        raise


def dgrad_bnb(dy, wpacked_ptr, layout, cout, ksize, bn_y, bn_ss, bn_mean, bn_relu, split=None, bn_second=False, tail=None,
              in_amax=None):
    """Data gradient (`wpacked_ptr`: the layer's data-gradient weights; layout 0 fp32, 1 x3, 2 the 16-channel x3 fragments) whose
    epilogue masks the result with the ReLU of the conv + BatchNorm layer it flows into and forms that layer's BatchNorm-backward
    reductions (include/wtpse_hip.h, wtpse_dgrad_bnb).  With a split the BatchNorm'd tensor is out0, or out1 if `bn_second`.
    tail = (gamma, invstd, dgamma, dbeta) of that BatchNorm: the launch also folds the partials and leaves the coefficients
    (wtpse_dgrad_bnb_coef).  A fifth element, dbias: that BatchNorm runs on frozen statistics — bn_mean / invstd are the running
    ones, the coefficients come out as (k1, 0, 0) and dbias receives the gradient of the conv bias in front of it
    (wtpse_dgrad_bnb_coef_frozen).
    -> (out0, out1 or None, stats [nblk, Cbn, 2], coef [Cbn, 3] or None)."""
    _chk(dy, "dy"); _chk(bn_y, "bn_y"); _chk(bn_ss, "bn_ss"); _chk(bn_mean, "bn_mean")
    layout = int(layout)
    B, C, H, W = dy.shape
    L = lib()
    out0, out1, csplit = _out_pair(split, B, cout, H, W, dy.device)
    c0, c1 = (csplit, cout) if (bn_second and split is not None) else (0, csplit)
    assert bn_y.shape == (B, c1 - c0, H, W), (bn_y.shape, (B, c1 - c0, H, W))
    nblk = _stats_blocks(layout, B, H, W, cout, ksize)
    stats = torch.empty((nblk, c1 - c0, 2), dtype=torch.float32, device=dy.device)
    if tail is not None:
        gamma, invstd, dgamma, dbeta = tail[:4]
        coef = torch.empty((c1 - c0, 3), dtype=torch.float32, device=dy.device)
        partial2 = torch.empty(L.query("wtpse_bnb_tail_partial2", nblk, cout), dtype=torch.float64, device=dy.device)
        tickets, tview = _tickets(L.query("wtpse_bnb_tail_tickets", nblk, cout), dy.device)
        frozen = len(tail) == 5
        args = [ptr(dy), C, wpacked_ptr, layout, ptr(out0), ptr(out1), csplit, ptr(bn_y), ptr(bn_ss), ptr(bn_mean), int(bool(bn_relu)),
                c0, c1, ptr(stats), ptr(gamma), ptr(invstd), ptr(coef), ptr(dgamma), ptr(dbeta)] + ([ptr(tail[4])] if frozen else [])
        _ticket_call(tview, "wtpse_dgrad_bnb_coef_frozen" if frozen else "wtpse_dgrad_bnb_coef", *args, 0, ptr(partial2), tickets,
                     B, H, W, cout, ksize, ptr(in_amax), stream_ptr())
        return out0, out1, stats, coef
    if layout == 2:
        L.call("wtpse_conv16_x3", ptr(dy), C, wpacked_ptr, 0, 0, 0, ptr(out0), ptr(stats), 0, ptr(bn_y), ptr(bn_ss), ptr(bn_mean),
               int(bool(bn_relu)), B, H, W, cout, 0, 1, ptr(in_amax), 0, stream_ptr())
    elif layout == 1:
        L.call("wtpse_dgrad_x3_bnb", ptr(dy), C, wpacked_ptr, ptr(out0), ptr(out1), csplit, ptr(bn_y), ptr(bn_ss), ptr(bn_mean),
               int(bool(bn_relu)), c0, c1, ptr(stats), B, H, W, cout, ksize, ptr(in_amax), stream_ptr())
    else:
        L.call("wtpse_dgrad_bnb", ptr(dy), C, wpacked_ptr, ptr(out0), ptr(out1), csplit,
               ptr(bn_y), ptr(bn_ss), ptr(bn_mean), int(bool(bn_relu)), c0, c1, ptr(stats), B, H, W, cout, ksize, stream_ptr())
    return out0, out1, stats, None


def _wgrad_prelude(query, dy, x0, x1, taps, want_dbias=False):
    """The prelude of the weight-gradient wrappers, for dy [B,cout,H,W] and the inputs x0 (, x1): the slab count the family's size
    `query` gives and the workspaces of that many slabs -> (lib, n, slab, dbias_slab | None, B, cout, H, W, C0, C1)."""
    _chk(dy, "dy"); _chk(x0, "x0"); _chk(x1, "x1")
    B, cout, H, W = dy.shape
    L, C0, C1 = lib(), x0.shape[1], 0 if x1 is None else x1.shape[1]
    n = L.query(query, B, H, W, C0 + C1, cout)
    slab = workspace("wgrad_slab", n * cout * (C0 + C1) * taps, dy.device)
    dbs = workspace("wgrad_dbias", n * cout, dy.device) if want_dbias else None
    return L, n, slab, dbs, B, cout, H, W, C0, C1


def conv_wgrad(dy, x0, x1, ksize, dw, dbias, pro0=None, pro_relu=0, accumulate=False, pro1=None):
    """dw / dbias are views into the flat gradient buffer ([Cout,Cin,k,k] / [Cout] or None)."""
    L, ks, slab, dbs, B, cout, H, W, C0, C1 = _wgrad_prelude("wtpse_wgrad_ksplit", dy, x0, x1, ksize * ksize, dbias is not None)
    L.call("wtpse_conv_wgrad", ptr(dy), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), int(pro_relu), ptr(slab), ptr(dbs), ks,
           ptr(dw), ptr(dbias), int(accumulate), B, H, W, cout, ksize, stream_ptr())


def wgrad_x3_supported(cin, cout, ksize, c0):
    return bool(lib().query("wtpse_wgrad_x3_supported", int(cin), int(cout), int(ksize), int(c0)))


def conv_wgrad_x3(dy, x0, x1, ksize, dw, pro0=None, pro_relu=0, accumulate=False, pro1=None):
    """conv_wgrad in the x3 arithmetic (csrc/conv_x3.hip); no bias gradient."""
    L, ks, slab, _, B, cout, H, W, C0, C1 = _wgrad_prelude("wtpse_wgrad_x3_ksplit", dy, x0, x1, ksize * ksize)
    L.call("wtpse_conv_wgrad_x3", ptr(dy), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), int(pro_relu), ptr(slab), ks, ptr(dw),
           int(accumulate), B, H, W, cout, ksize, stream_ptr())


def wgrad_r_supported(cin, cout, ksize, c0, w):
    return bool(lib().query("wtpse_wgrad_r_supported", int(cin), int(cout), int(ksize), int(c0), int(w)))


def conv_wgrad_r(dy, x0, x1, dw, dbias=None, pro0=None, pro_relu=0, accumulate=False, pro1=None, dy_amax=None, x_amax0=None,
                 x_amax1=None):
    """3x3 conv_wgrad in the x3 arithmetic with register-resident operands (csrc/wgrad_r.hip); with bias gradient.
    dy_amax: amax_of(dy) (x2h: the scale of the gradient operand); x_amax0 / x_amax1: the bounds of x0 / x1 as loaded."""
    L, ns, slab, dbs, B, cout, H, W, C0, C1 = _wgrad_prelude("wtpse_wgrad_r_slabs", dy, x0, x1, 9, dbias is not None)
    L.call("wtpse_conv_wgrad_r", ptr(dy), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), int(pro_relu), ptr(slab), ptr(dbs), ns,
           ptr(dw), ptr(dbias), int(accumulate), B, H, W, cout, ptr(dy_amax), ptr(x_amax0), ptr(x_amax1), stream_ptr())


def conv_wgrad_r_bn(g, bn_y, coef, x0, x1, dw, pro0=None, pro_relu=0, accumulate=False, pro1=None):
    """conv_wgrad_r with dY = coef[:,0] * g + coef[:,1] * bn_y + coef[:,2] formed on load (no bias gradient)."""
    _chk(bn_y, "bn_y")
    L, ns, slab, _, B, cout, H, W, C0, C1 = _wgrad_prelude("wtpse_wgrad_r_slabs", g, x0, x1, 9)
    L.call("wtpse_conv_wgrad_r_bn", ptr(g), ptr(bn_y), ptr(coef), ptr(x0), C0, ptr(x1), C1, ptr(pro0), ptr(pro1), int(pro_relu),
           ptr(slab), ns, ptr(dw), int(accumulate), B, H, W, cout, stream_ptr())


# ----------------------------------------------------------------------------------------------- batch norm
def conv_fwd_bnf(in0, in1, wpacked_ptr, layout, bias, cout, ksize, pro0, pro_relu, pro1, gamma, beta, rmean, rvar, nbt,
                 momentum=0.1, eps=1e-5, in_amax0=None, in_amax1=None, act_amax=None):
    """Forward convolution in front of a train-mode BatchNorm, statistics finished by the same launch (include/wtpse_hip.h,
    wtpse_conv_fwd_bnf).  layout 0 fp32, 1 x3, 2 the 16-channel x3 fragments.  in_amax0 / in_amax1: the bounds of the inputs as
    loaded; act_amax: a zeroed table that receives the bound of the BatchNorm's output.  -> (y, ss [C,2], mean, invstd)."""
    _chk(in0, "in0"); _chk(in1, "in1"); _chk(pro0, "pro0"); _chk(pro1, "pro1")
    layout = int(layout)
    B, C0, H, W = in0.shape
    C1 = 0 if in1 is None else in1.shape[1]
    L = lib()
    dev = in0.device
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=dev)
    nblk = _stats_blocks(layout, B, H, W, cout, ksize)
    stats = torch.empty((nblk, cout, 2), dtype=torch.float32, device=dev)
    ss = torch.empty((cout, 2), dtype=torch.float32, device=dev)
    mean = torch.empty((cout,), dtype=torch.float32, device=dev)
    invstd = torch.empty((cout,), dtype=torch.float32, device=dev)
    partial2 = torch.empty(L.query("wtpse_bnb_tail_partial2", nblk, cout), dtype=torch.float64, device=dev)
    tickets, tview = _tickets(L.query("wtpse_bnb_tail_tickets", nblk, cout), dev)
    _ticket_call(tview, "wtpse_conv_fwd_bnf", ptr(in0), C0, ptr(in1), C1, wpacked_ptr, layout, ptr(bias), ptr(pro0), ptr(pro1), int(pro_relu),
           ptr(out), ptr(stats), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), ptr(nbt), float(momentum), float(eps), ptr(ss),
           ptr(mean), ptr(invstd), ptr(partial2), tickets, B, H, W, cout, ksize, ptr(in_amax0), ptr(in_amax1), ptr(act_amax),
           stream_ptr())
    return out, ss, mean, invstd


def bn_finalize(stats, count, gamma, beta, rmean, rvar, nbt, momentum=0.1, eps=1e-5, act_amax=None):
    nblk, C, _ = stats.shape
    dev = stats.device
    ss = torch.empty((C, 2), dtype=torch.float32, device=dev)
    mean = torch.empty((C,), dtype=torch.float32, device=dev)
    invstd = torch.empty((C,), dtype=torch.float32, device=dev)
    lib().call("wtpse_bn_finalize", ptr(stats), nblk, C, int(count), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar),
               ptr(nbt), float(momentum), float(eps), ptr(ss), ptr(mean), ptr(invstd), ptr(act_amax), stream_ptr())
    return ss, mean, invstd


def bn_finalize_blend(stats, count, gamma, beta, rmean, rvar, w, eps=1e-5, acc=None, acc_count=0, moments=None, div=None, act_amax=None):
    """Eval-mode scale / shift on target statistics (include/wtpse_hip.h, wtpse_bn_finalize_blend; adapt.py is the specification): the
    partials `stats` of this call's `count` values per channel, pooled with acc (float64 [C,2], updated in place; acc_count values seen
    before) and blended with the running statistics at weight w.  rmean / rvar are read only.  moments (float64 [C,4]), div (float64
    [C]) and act_amax (a zeroed amax table) are filled when given.  -> ss [C,2]."""
    nblk, C, _ = stats.shape
    for t, shape in ((acc, (C, 2)), (moments, (C, 4)), (div, (C,))):
        if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError("bn_finalize_blend: acc / moments / div must be contiguous float64 device tensors [C,2] / [C,4] / [C]")
    ss = torch.empty((C, 2), dtype=torch.float32, device=stats.device)
    lib().call("wtpse_bn_finalize_blend", ptr(stats), nblk, C, int(count), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(w),
               float(eps), ptr(acc), float(acc_count), ptr(ss), ptr(moments), ptr(div), ptr(act_amax), stream_ptr())
    return ss


def bn_eval_coeffs(gamma, beta, rmean, rvar, eps=1e-5):
    C = gamma.numel()
    ss = torch.empty((C, 2), dtype=torch.float32, device=gamma.device)
    lib().call("wtpse_bn_eval_coeffs", ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(eps), C, ptr(ss), stream_ptr())
    return ss


def bn_eval_coeffs_stats(gamma, beta, rmean, rvar, eps=1e-5):
    """bn_eval_coeffs plus what a backward through the eval-mode BatchNorm takes for the batch statistics: -> (ss, mean, invstd) with
    mean = the running mean, invstd = 1 / sqrt(running_var + eps)."""
    C = gamma.numel()
    ss = torch.empty((C, 2), dtype=torch.float32, device=gamma.device)
    mean = torch.empty((C,), dtype=torch.float32, device=gamma.device)
    invstd = torch.empty((C,), dtype=torch.float32, device=gamma.device)
    lib().call("wtpse_bn_eval_coeffs_stats", ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(eps), C, ptr(ss), ptr(mean),
               ptr(invstd), stream_ptr())
    return ss, mean, invstd


def affine_act(y, ss, relu):
    _chk(y, "y")
    B, C, H, W = y.shape
    z = torch.empty_like(y)
    lib().call("wtpse_affine_act", ptr(y), ptr(ss), int(relu), ptr(z), B, C, H * W, stream_ptr())
    return z


def _dy_like(t):
    """The dy of a BatchNorm backward: shaped like t, with the amax table its x2h consumers read (filled by the launch)."""
    dy = torch.empty_like(t)
    amax_attach(dy, _amax_table(t.device))
    return dy


def bn_bwd(dz, y, ss, relu, gamma, mean, invstd, dgamma, dbeta, accumulate=False):
    _chk(dz, "dz"); _chk(y, "y")
    B, C, H, W = y.shape
    L = lib()
    ns = L.query("wtpse_bn_bwd_nsplit", B, C, H * W)
    partial = workspace("bn_bwd_partial", ns * C * 2, y.device)
    coef = workspace("bn_bwd_coef", C * 3, y.device)
    dy = _dy_like(y)
    L.call("wtpse_bn_bwd", ptr(dz), ptr(y), ptr(ss), int(relu), ptr(gamma), ptr(mean), ptr(invstd), ptr(partial),
           ptr(coef), ptr(dgamma), ptr(dbeta), int(accumulate), ptr(dy), B, C, H * W, ptr(dy.wt_amax), stream_ptr())
    return dy


def bn_bwd_from_stats(g, y, stats, gamma, mean, invstd, dgamma, dbeta, accumulate=False):
    """Second half of a BatchNorm backward after dgrad_bnb: g = masked incoming gradient, stats = its partials.  -> dy."""
    _chk(g, "g"); _chk(y, "y"); _chk(stats, "stats")
    B, C, H, W = y.shape
    assert stats.shape[1] == C
    coef = workspace("bn_bwd_coef", C * 3, y.device)
    dy = _dy_like(y)
    lib().call("wtpse_bn_bwd_from_stats", ptr(g), ptr(y), ptr(stats), stats.shape[0], ptr(gamma), ptr(mean), ptr(invstd), ptr(coef),
               ptr(dgamma), ptr(dbeta), int(accumulate), ptr(dy), B, C, H * W, ptr(dy.wt_amax), stream_ptr())
    return dy


# ---- frozen statistics: the backward through an eval-mode BatchNorm (include/wtpse_hip.h, wtpse_bn_bwd_frozen).  mean / invstd:
# from bn_eval_coeffs_stats; dbias: the gradient view of the bias of the convolution in front of the BatchNorm.
def bn_bwd_frozen(dz, y, ss, relu, gamma, mean, invstd, dgamma, dbeta, dbias, accumulate=False):
    _chk(dz, "dz"); _chk(y, "y")
    B, C, H, W = y.shape
    L = lib()
    ns = L.query("wtpse_bn_bwd_nsplit", B, C, H * W)
    partial = workspace("bn_bwd_partial", ns * C * 2, y.device)
    coef = workspace("bn_bwd_coef", C * 3, y.device)
    dy = _dy_like(y)
    L.call("wtpse_bn_bwd_frozen", ptr(dz), ptr(y), ptr(ss), int(relu), ptr(gamma), ptr(mean), ptr(invstd), ptr(partial), ptr(coef),
           ptr(dgamma), ptr(dbeta), ptr(dbias), int(accumulate), ptr(dy), B, C, H * W, ptr(dy.wt_amax), stream_ptr())
    return dy


def bn_bwd_from_stats_frozen(g, stats, gamma, invstd, dgamma, dbeta, dbias, accumulate=False):
    """g = masked incoming gradient, stats = its partials against the running mean (dgrad_bnb / maxpool2_bwd_bnb).  -> dy."""
    _chk(g, "g"); _chk(stats, "stats")
    B, C, H, W = g.shape
    assert stats.shape[1] == C
    coef = workspace("bn_bwd_coef", C * 3, g.device)
    dy = _dy_like(g)
    lib().call("wtpse_bn_bwd_from_stats_frozen", ptr(g), ptr(stats), stats.shape[0], ptr(gamma), ptr(invstd), ptr(coef), ptr(dgamma),
               ptr(dbeta), ptr(dbias), int(accumulate), ptr(dy), B, C, H * W, ptr(dy.wt_amax), stream_ptr())
    return dy


def bn_bwd_finalize_coef_frozen(stats, gamma, invstd, dgamma, dbeta, dbias, accumulate=False):
    """The fold alone: partials -> coef [C, 3] = (k1, 0, 0), dgamma / dbeta / dbias."""
    _chk(stats, "stats")
    C = stats.shape[1]
    coef = torch.empty((C, 3), dtype=torch.float32, device=stats.device)
    lib().call("wtpse_bn_bwd_finalize_coef_frozen", ptr(stats), stats.shape[0], C, ptr(gamma), ptr(invstd), ptr(coef), ptr(dgamma),
               ptr(dbeta), ptr(dbias), int(accumulate), stream_ptr())
    return coef


def bn_bwd_scale_coef(g, coef):
    """dy = k1 g with the coefficients a frozen dgrad_bnb(..., tail=) launch left (k2 = k3 = 0: y is not read)."""
    _chk(g, "g"); _chk(coef, "coef")
    B, C, H, W = g.shape
    dy = _dy_like(g)
    lib().call("wtpse_bn_bwd_scale_coef", ptr(g), ptr(coef), ptr(dy), B, C, H * W, ptr(dy.wt_amax), stream_ptr())
    return dy


def bn_frozen_fold_spec(g, y, gamma, running_mean, running_var, eps=1e-5):
    """Host specification of the frozen fold (any device, any float dtype; the tests hold the kernels and torch's autograd of
    F.batch_norm(training=False) against it): g = the gradient already masked with the layer's ReLU, y = the raw conv output,
    both [B, C, H, W].  -> (dy, dgamma, dbeta, dbias, mean, invstd)."""
    r = 1.0 / torch.sqrt(running_var + eps)
    s = gamma * r
    sum_g = g.sum(dim=(0, 2, 3))
    sum_gy = (g * (y - running_mean.view(1, -1, 1, 1))).sum(dim=(0, 2, 3))
    return s.view(1, -1, 1, 1) * g, r * sum_gy, sum_g, s * sum_g, running_mean, r


# ----------------------------------------------------------------------------------------------- WT loss
class WtLossState:
    __slots__ = ("z", "gram", "offdiag", "diag", "dmmd_dv", "losses", "v", "B", "HW", "D", "n", "margin")


def bn_bwd_apply_coef(g, y, coef):
    """dy = k1 g + k2 y + k3 with the coefficients a dgrad_bnb(..., tail=) launch left."""
    _chk(g, "g"); _chk(y, "y")
    B, C, H, W = y.shape
    dy = _dy_like(y)
    lib().call("wtpse_bn_bwd_apply_coef", ptr(g), ptr(y), ptr(coef), ptr(dy), B, C, H * W, ptr(dy.wt_amax), stream_ptr())
    return dy


def wt_loss_fwd(z, domain_num, per_domain, margin=0.0, eps=1e-5, losses_out=None, gram_partial=None):
    """-> WtLossState; st.losses = device [3] = (ins_offdiag, ins_diag, domain).
    gram_partial: (partial, S) from conv_fwd_gram — the producer of z already formed the per-tile Grams: z is not read."""
    _chk(z, "z")
    B, C, H, W = z.shape
    HW = H * W
    dev = z.device
    L = lib()
    S = L.query("wtpse_wt_split", B, HW, 0)
    R = domain_num * per_domain
    st = WtLossState()
    partial = workspace("wt_partial", B * S * 256, dev) if gram_partial is None else None
    st.gram = torch.empty((B, 256), dtype=torch.float32, device=dev)
    st.v = torch.empty((B, 120), dtype=torch.float32, device=dev)
    st.offdiag = torch.empty((B,), dtype=torch.float32, device=dev)
    st.diag = torch.empty((B,), dtype=torch.float32, device=dev)
    rowval = torch.empty((max(R, 1) + 1,), dtype=torch.float64, device=dev)     # + the tail launch's ticket word
    st.dmmd_dv = torch.empty((max(R, 1), 120), dtype=torch.float32, device=dev)
    st.losses = losses_out if losses_out is not None else torch.empty((3,), dtype=torch.float32, device=dev)
    if gram_partial is not None:
        gp, gs = gram_partial
        assert C == 16 and gp.shape[0] == B * gs
        L.call("wtpse_wt_loss_fwd_partials", ptr(gp), int(gs), B, HW, float(eps), float(margin), int(domain_num), int(per_domain),
               ptr(st.gram), ptr(st.v), ptr(st.offdiag), ptr(st.diag), ptr(rowval), ptr(st.dmmd_dv), ptr(st.losses), stream_ptr())
    else:
        L.call("wtpse_wt_loss_fwd", ptr(z), B, C, HW, float(eps), float(margin), int(domain_num), int(per_domain),
               ptr(partial), ptr(st.gram), ptr(st.v), ptr(st.offdiag), ptr(st.diag), ptr(rowval), ptr(st.dmmd_dv),
               ptr(st.losses), stream_ptr())
    st.z, st.B, st.HW, st.D, st.n, st.margin = z, B, HW, domain_num, per_domain, float(margin)
    return st


def wt_loss_bwd(st, dz, accumulate, g_off=None, g_diag=None, g_dom=None, w_off=1.0, w_diag=1.0, w_dom=1.0):
    _chk(dz, "dz")
    _amax_stale(dz)
    Mws = workspace("wt_M", st.B * 256, dz.device)
    lib().call("wtpse_wt_loss_bwd", ptr(st.z), st.B, 16, st.HW, st.margin, st.D, st.n, ptr(st.gram), ptr(st.offdiag),
               ptr(st.diag), ptr(st.dmmd_dv), ptr(g_off), ptr(g_diag), ptr(g_dom), float(w_off), float(w_diag),
               float(w_dom), ptr(Mws), ptr(dz), int(accumulate), stream_ptr())


def wt_combine(losses, den, mode, out=None):
    """losses [nmaps,3] -> out[4] = (ins_total, ins_off, ins_diag, dom); mode 1 = student accumulator quirk."""
    if out is None:
        out = torch.empty((4,), dtype=torch.float32, device=losses.device)
    lib().call("wtpse_wt_combine", ptr(losses), losses.shape[0], float(den), int(mode), ptr(out), stream_ptr())
    return out


# ----------------------------------------------------------------------------------------------- pooling etc.
def maxpool2_fwd(x, pro=None, relu=False):
    _chk(x, "x")
    B, C, H, W = x.shape
    out = torch.empty((B, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    lib().call("wtpse_maxpool2_fwd", ptr(x), ptr(pro), int(relu), ptr(out), B, C, H, W, stream_ptr())
    return out


def maxpool2_bwd(x, dout, dx, accumulate, pro=None, relu=False, mask=False):
    """mask: the result is also multiplied with [act(x) > 0] (the ReLU that produced x)."""
    B, C, H, W = x.shape
    if dx is None:
        dx = torch.empty_like(x)
        accumulate = False
    _amax_stale(dx)
    lib().call("wtpse_maxpool2_bwd", ptr(x), ptr(pro), int(relu), ptr(dout), ptr(dx), int(bool(accumulate)) | (2 if mask else 0),
               B, C, H, W, stream_ptr())
    return dx


def maxpool2_bwd_bnb(x, dout, dx, pro, relu, mean):
    """maxpool2_bwd(mask=True) on the raw output of a conv + BatchNorm + ReLU layer that also forms the BatchNorm-backward
    reductions of that layer.  -> (masked gradient, stats [nblk, C, 2]) or None when the shape is not supported."""
    B, C, H, W = x.shape
    if W % 4 or H % 2 or B * C >= 32768 or pro is None:
        return None
    L = lib()
    acc = dx is not None
    if dx is None:
        dx = torch.empty_like(x)
    _amax_stale(dx)
    stats = torch.empty((L.query("wtpse_maxpool2_bwd_stats_blocks", B, H, W), C, 2), dtype=torch.float32, device=x.device)
    L.call("wtpse_maxpool2_bwd_bnb", ptr(x), ptr(pro), int(relu), ptr(dout), ptr(dx), int(acc), ptr(mean), ptr(stats), B, C, H, W,
           stream_ptr())
    return dx, stats


def upsample2x_fwd(x, pro=None, relu=False):
    _chk(x, "x")
    B, C, H, W = x.shape
    out = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    lib().call("wtpse_upsample2x_fwd", ptr(x), ptr(pro), int(relu), ptr(out), B, C, H, W, stream_ptr())
    return out


def upsample2x_fwd_stats(x):
    """-> (out, stats [nblk, C, 2]): bilinear x2 plus the (sum, sum of squares) partials of the output."""
    _chk(x, "x")
    B, C, H, W = x.shape
    out = torch.empty((B, C, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    nblk = lib().query("wtpse_upsample2x_stats_blocks", B, H, W)
    stats = torch.empty((nblk, C, 2), dtype=torch.float32, device=x.device)
    lib().call("wtpse_upsample2x_fwd_stats", ptr(x), ptr(out), ptr(stats), B, C, H, W, stream_ptr())
    return out, stats


def upsample2x_bwd(dout):
    _chk(dout, "dout")
    B, C, Ho, Wo = dout.shape
    dx = torch.empty((B, C, Ho // 2, Wo // 2), dtype=torch.float32, device=dout.device)
    amax_attach(dx, _amax_table(dout.device))
    lib().call("wtpse_upsample2x_bwd", ptr(dout), ptr(dx), 0, B, C, Ho // 2, Wo // 2, ptr(dx.wt_amax), stream_ptr())
    return dx


def upsample2x_bwd_bn(g, bn_y, coef):
    """upsample2x_bwd of dout = coef[:,0] * g + coef[:,1] * bn_y + coef[:,2] formed on load (no apply pass, dout never written)."""
    _chk(g, "g"); _chk(bn_y, "bn_y"); _chk(coef, "coef")
    B, C, Ho, Wo = g.shape
    assert bn_y.shape == g.shape and coef.shape == (C, 3) and Wo % 8 == 0, (g.shape, bn_y.shape, coef.shape)
    dx = torch.empty((B, C, Ho // 2, Wo // 2), dtype=torch.float32, device=g.device)
    amax_attach(dx, _amax_table(g.device))
    lib().call("wtpse_upsample2x_bwd_bn", ptr(g), ptr(bn_y), ptr(coef), ptr(dx), B, C, Ho // 2, Wo // 2, ptr(dx.wt_amax), stream_ptr())
    return dx


def resize_bilinear(x, size):
    _chk(x, "x")
    B, C, H, W = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device)
    lib().call("wtpse_resize_bilinear", ptr(x), ptr(out), B, C, H, W, Ho, Wo, stream_ptr())
    return out


def relu_mask(dz, ref, out=None, accumulate=False):
    _chk(dz, "dz"); _chk(ref, "ref")
    if out is None:
        out = torch.empty_like(dz)
        accumulate = False
    _amax_stale(out)
    lib().call("wtpse_relu_mask", ptr(dz), ptr(ref), ptr(out), int(accumulate), dz.numel(), stream_ptr())
    return out


def _amax_stale(t):
    """t is about to be modified in place: an amax table its producer attached no longer describes it."""
    if t is not None and getattr(t, "wt_amax", None) is not None:
        t.wt_amax = None


def axpy(dst, src, alpha=1.0):
    _amax_stale(dst)
    lib().call("wtpse_axpy", ptr(dst), ptr(src), float(alpha), dst.numel(), stream_ptr())
    return dst


def zero_(t):
    _amax_stale(t)
    lib().call("wtpse_zero", ptr(t), t.numel() * t.element_size(), stream_ptr())
    return t


# ----------------------------------------------------------------------------------------------- fused 1x1 heads
def head_fwd(x, pro, relu, w1, b1, w2, b2, w3, b3, want_tape=True, x_amax=None, want_h1=False):
    """32 -> 32 (ReLU) -> 8 [-> (ReLU) -> nc] in one kernel.  -> (out, h1 or None, h2): out is y [B,nc,H,W] for a
    three-layer head (w3 given), the 8-channel h2 for a two-layer head."""
    _chk(x, "x"); _chk(pro, "pro")
    B, C, H, W = x.shape
    three = w3 is not None
    nc = w3.shape[0] if three else 0
    # (x2h arithmetic: the backward forms layer 1 again from x — no h1 tape, 128 bytes per pixel less written here and read there)
    h1 = torch.empty((B, 32, H, W), dtype=torch.float32, device=x.device) if (want_tape and (want_h1 or x3_terms() != 2)) else None
    h2 = torch.empty((B, 8, H, W), dtype=torch.float32, device=x.device) if (want_tape or not three) else None
    y = torch.empty((B, nc, H, W), dtype=torch.float32, device=x.device) if three else None
    lib().call("wtpse_head_fwd", ptr(x), ptr(pro), int(bool(relu)), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), nc,
               ptr(h1), ptr(h2), ptr(y), ptr(x_amax), B, H * W, stream_ptr())
    return (y if three else h2), h1, h2


def head_bwd(dy, x, pro, relu, h1, h2, w1, w2, w3, dparams, accumulate=False, b1=None, x_amax=None, dy_amax=None):
    """-> dx (gradient wrt the activated input); the parameter gradients land in `dparams`, the contiguous flat-buffer
    range (dW1, db1, dW2, db2[, dW3, db3]).  x2h arithmetic (the default): h1 is not read — the kernel forms layer 1 again from
    x (b1 required) — and the operand scales come from the amax tables of the activated x (None: the fixed forward scale) and
    of dy (None: one extra pass over dy here); otherwise the fp32-input kernel, which reads the h1 tape."""
    _chk(dy, "dy"); _chk(x, "x"); _chk(h1, "h1"); _chk(h2, "h2")
    if x3_terms() == 2:
        if b1 is None:
            raise ValueError("head_bwd (x2h): b1 is required — layer 1 is formed again from x")
        if dy_amax is None:
            dy_amax = amax_of(dy)
    elif h1 is None:
        raise ValueError("head_bwd: the fp32-input kernel reads the layer-1 tape h1 (head_fwd(..., want_h1=True))")
    B, C, H, W = x.shape
    nc = w3.shape[0] if w3 is not None else 0
    L = lib()
    ns = 1024 + 32 + 256 + 8 + 9 * nc
    assert dparams.numel() == ns and dparams.is_contiguous()
    _amax_stale(dparams)
    slab = workspace("head_slab", L.query("wtpse_head_slabs", B, H * W) * ns, x.device)
    dx = torch.empty_like(x)
    L.call("wtpse_head_bwd", ptr(dy), ptr(x), ptr(pro), int(bool(relu)), ptr(h1), ptr(h2), ptr(w1), ptr(b1), ptr(w2), ptr(w3), nc,
           ptr(dx), ptr(slab), ptr(dparams), int(accumulate), ptr(x_amax), ptr(dy_amax), B, H * W, stream_ptr())
    return dx


# ----------------------------------------------------------------------------------------------- attention / sampling
def attn_fuse_fwd(z, wb_ptr, emb, coef, want_att=True, want_pre=False, want_mask=False):
    _chk(z, "z"); _chk(emb, "emb")
    B, CE, H, W = emb.shape
    att = torch.empty_like(z) if want_att else None
    pre = torch.empty_like(z) if want_pre else None
    mask = torch.empty_like(z) if want_mask else None
    fuse = torch.empty_like(emb)
    lib().call("wtpse_attn_fuse_fwd", ptr(z), wb_ptr, ptr(emb), float(coef), ptr(att), ptr(pre), ptr(mask), ptr(fuse),
               B, CE, H * W, stream_ptr())
    return att, pre, mask, fuse


def attn_fuse_bwd(dfuse, z, emb, att, wb_ptr, coef, d_wb_ptr, want_dz=True, accumulate=False):
    B, CE, H, W = emb.shape
    demb = torch.empty_like(emb)
    dz = torch.empty_like(z) if want_dz else None
    nb = (B * H * W + 255) // 256
    partial = workspace("attn_partial", 2 * nb, emb.device)
    lib().call("wtpse_attn_fuse_bwd", ptr(dfuse), ptr(z), ptr(emb), ptr(att), wb_ptr, float(coef), ptr(demb), ptr(dz),
               ptr(partial), d_wb_ptr, int(accumulate), B, CE, H * W, stream_ptr())
    return demb, dz


def reparam_fwd(mu, logvar, eps):
    z = torch.empty_like(mu)
    lib().call("wtpse_reparam_fwd", ptr(mu), ptr(logvar), ptr(eps), ptr(z), mu.numel(), stream_ptr())
    return z


def reparam_bwd(dz, logvar, eps):
    dlv = torch.empty_like(dz)
    lib().call("wtpse_reparam_bwd", ptr(dz), ptr(logvar), ptr(eps), ptr(dlv), dz.numel(), stream_ptr())
    return dlv


def reparam_student(mu, logvar, eps, flag):
    std = torch.empty_like(mu)
    lib().call("wtpse_exp_half", ptr(logvar), ptr(std), mu.numel(), stream_ptr())
    nan_scrub_(std, flag)
    z = torch.empty_like(mu)
    lib().call("wtpse_reparam_student", ptr(mu), ptr(std), ptr(eps), ptr(z), mu.numel(), stream_ptr())
    return z


def nan_scrub_(x, flag):
    _amax_stale(x)
    lib().call("wtpse_nan_scrub", ptr(x), x.numel(), flag.data_ptr(), stream_ptr())
    return x


def randn(shape, device, seed, offset=0, offset_dev=None):
    """Standard normals from the Philox stream `seed` at position offset + *offset_dev (device uint64 counter or None)."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    lib().call("wtpse_randn", ptr(out), out.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), ptr(offset_dev), stream_ptr())
    return out


def shape_samples(emb, mu, logvar, wb_ptr, coef, wout_ptr, bout_ptr, wz_ptr, n_samples, seed=0, offset=0, scale=1.0, noise=None,
                  threshold=0.75, want_logits=False, image_stride=None):
    """K = n_samples draws of the latent and everything behind it in one launch (csrc/uncertainty.hip; uncertainty.shape_samples_host
    is its specification): emb [B,CE,H,W], mu / logvar [B,1,H,W]; wb_ptr -> {w, b} of the attention layer, wout_ptr -> [CE] and
    bout_ptr -> [1] of the output convolution, wz_ptr -> the latent's own weight (cat_shape) or 0.  eps[b,k] is the H*W elements
    of the ops.randn stream `seed` from offset + (b*K + k)*H*W on, or noise[b,k] when noise [B,K,H,W] is given.
    -> (mean, std [B,1,H,W] fp32, votes [B,1,H,W] uint8, logits [B,K,H,W] or None).
    image_stride (elements, a multiple of 4): image b draws from offset + b*image_stride instead of offset + b*K*H*W — one launch per
    image then, on views of the same tensors (the kernel's stream layout is dense)."""
    _chk(emb, "emb"); _chk(mu, "mu"); _chk(logvar, "logvar"); _chk(noise, "noise")
    B, CE, H, W = emb.shape
    K, HW = int(n_samples), H * W
    if mu.numel() != B * HW or logvar.numel() != B * HW:
        raise ValueError("mu %s / logvar %s do not match emb %s" % (tuple(mu.shape), tuple(logvar.shape), tuple(emb.shape)))
    if noise is not None and tuple(noise.shape) != (B, K, H, W):
        raise ValueError("noise must be [B,K,H,W] = %s (got %s)" % ((B, K, H, W), tuple(noise.shape)))
    dev = emb.device
    mean = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    std = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    votes = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    logits = torch.empty((B, K, H, W), dtype=torch.float32, device=dev) if want_logits else None
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    def launch(sl, off, nb):
        v = lambda t: 0 if t is None else t[sl].data_ptr()
        lib().call("wtpse_shape_samples", v(emb), CE, v(mu), v(logvar), wb_ptr, float(coef), wout_ptr, bout_ptr, wz_ptr, float(scale), K,
                   seed, int(off), v(noise), float(threshold), v(mean), v(std), v(votes), v(logits), nb, HW, stream_ptr())

    if image_stride is None or int(image_stride) == K * HW or B == 1:
        launch(slice(0, B), offset, B)
    else:
        for b in range(B):
            launch(slice(b, b + 1), int(offset) + b * int(image_stride), 1)
    return mean, std, votes, logits


def shape_samples_mask_(ref, mean, std, votes, logits=None):
    """In place, what shape_samples would have left had every sampled logit been multiplied by the {0,1} map ref [B,1,H,W] first (the
    cup's logits times od_pred): where ref <= 0, logits 0, mean 0.5, std 0, votes 0."""
    _chk(ref, "ref"); _chk(mean, "mean"); _chk(std, "std"); _chk(logits, "logits")
    B, _, H, W = mean.shape
    K = 1 if logits is None else logits.shape[1]
    if not (ref.numel() == mean.numel() == std.numel() == votes.numel() and votes.dtype == torch.uint8 and votes.is_contiguous()):
        raise ValueError("shape_samples_mask_: ref, mean, std and votes (uint8) must be [B,1,H,W] of one size")
    for t in (mean, std, logits):
        _amax_stale(t)
    lib().call("wtpse_shape_samples_mask", ptr(ref), ptr(mean), ptr(std), ptr(votes), ptr(logits), K, B, H * W, stream_ptr())


def counter_add(counter, inc):
    """*counter += inc on the current stream (device int32 or int64 scalar tensor)."""
    lib().call("wtpse_counter_add", ptr(counter), int(inc), int(counter.dtype == torch.int64), stream_ptr())


# ----------------------------------------------------------------------------------------------- losses / optimiser
def _red_ws(n, device, mult=1):
    nb = lib().query("wtpse_reduce_blocks", n)
    return workspace("loss_partial", nb * mult, device)


def bce_sigmoid_fwd(x, t):
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    lib().call("wtpse_bce_sigmoid_fwd", ptr(x), ptr(t), x.numel(), ptr(_red_ws(x.numel(), x.device)), ptr(loss), stream_ptr())
    return loss


def bce_sigmoid_bwd(x, t, g=None, w=1.0):
    dx = torch.empty_like(x)
    lib().call("wtpse_bce_sigmoid_bwd", ptr(x), ptr(t), ptr(g), float(w), x.numel(), ptr(dx), stream_ptr())
    return dx


def pos_weight_sums(mask, t):
    """device [2] = (sum mask, sum mask*t) of THIS rank's rows (all-reduce before pos_weight_from_sums under DP)."""
    sums = torch.empty((2,), dtype=torch.float32, device=mask.device)
    pw = torch.empty((), dtype=torch.float32, device=mask.device)
    lib().call("wtpse_pos_weight", ptr(mask), ptr(t), mask.numel(), ptr(_red_ws(mask.numel(), mask.device, 2)), ptr(sums),
               ptr(pw), stream_ptr())
    return sums, pw


def pos_weight_from_sums(sums):
    pw = torch.empty((), dtype=torch.float32, device=sums.device)
    lib().call("wtpse_pos_weight_from_sums", ptr(sums), ptr(pw), stream_ptr())
    return pw


def bce_logits_pw_fwd(x, mask, t, pw):
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    lib().call("wtpse_bce_logits_pw_fwd", ptr(x), ptr(mask), ptr(t), ptr(pw), x.numel(), ptr(_red_ws(x.numel(), x.device)),
               ptr(loss), stream_ptr())
    return loss


def bce_logits_pw_bwd(x, mask, t, pw, g=None, w=1.0):
    dx = torch.empty_like(x)
    lib().call("wtpse_bce_logits_pw_bwd", ptr(x), ptr(mask), ptr(t), ptr(pw), ptr(g), float(w), x.numel(), ptr(dx), stream_ptr())
    return dx


def mse_fwd(a, b, out=None):
    loss = out if out is not None else torch.empty((), dtype=torch.float32, device=a.device)
    lib().call("wtpse_mse_fwd", ptr(a), ptr(b), a.numel(), ptr(_red_ws(a.numel(), a.device)), ptr(loss), stream_ptr())
    return loss


def mse_bwd(a, b, g=None, w=1.0):
    da = torch.empty_like(a)
    lib().call("wtpse_mse_bwd", ptr(a), ptr(b), ptr(g), float(w), a.numel(), ptr(da), stream_ptr())
    return da


def signed_distance(t, want_d2=False):
    """The signed distance map of every label plane of `t` (device fp32, [..., h, w], nonzero = object): phi of the same shape —
    boundary.signed_distance_host per plane, bit for bit float32 of it (wtpse_signed_distance).  want_d2: -> (phi, d2_out, d2_in)
    with the two exact squared-distance maps (int32, -1 where the set is empty)."""
    _chk(t, "t")
    if t.dim() < 2:
        raise ValueError("signed_distance: label planes [..., h, w], got shape %s" % (tuple(t.shape),))
    h, w = int(t.shape[-2]), int(t.shape[-1])
    B = t.numel() // max(h * w, 1)
    L = lib()
    words = L.query("wtpse_signed_distance_ws", B, h, w)
    if words <= 0:
        raise ValueError("signed_distance: unsupported size %s (1 <= h, w <= 4096)" % (tuple(t.shape),))
    phi = torch.empty_like(t)
    d2_out = torch.empty(t.shape, dtype=torch.int32, device=t.device) if want_d2 else None
    d2_in = torch.empty(t.shape, dtype=torch.int32, device=t.device) if want_d2 else None
    ws = workspace("signed_distance", words, t.device)
    L.call("wtpse_signed_distance", ptr(t), ptr(phi), ptr(d2_out), ptr(d2_in), ptr(ws), B, h, w, stream_ptr())
    return (phi, d2_out, d2_in) if want_d2 else phi


def boundary_loss(x, phi, alpha_dev, mask=None, dx=None):
    """-> the unweighted boundary loss mean(sigmoid(x * mask) * phi) (0-dim device fp32; mask None: the disc form).  With dx the same
    launch adds (*alpha_dev) / n * phi * s (1 - s) [* mask] into dx IN PLACE (alpha_dev: device fp32 scalar, read by the kernel)."""
    _chk(x, "x"); _chk(phi, "phi"); _chk(mask, "mask"); _chk(dx, "dx"); _chk(alpha_dev, "alpha_dev")
    n = x.numel()
    for name, v in (("phi", phi), ("mask", mask), ("dx", dx)):
        if v is not None and v.numel() != n:
            raise ValueError("boundary_loss: %s has %d elements, x has %d" % (name, v.numel(), n))
    if dx is not None and alpha_dev is None:
        raise ValueError("boundary_loss: dx needs the device weight alpha_dev")
    # phi reaches several hundred: an amax table that describes the region loss's gradient alone no longer bounds dx
    _amax_stale(dx)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    lib().call("wtpse_boundary_loss", ptr(x), ptr(mask), ptr(phi), ptr(alpha_dev), n, ptr(_red_ws(n, x.device)), ptr(loss), ptr(dx),
               stream_ptr())
    return loss


def overlap_loss(x, t, w_dev, cfg, mask=None, dx=None, want_planes=False):
    """-> the unweighted overlap loss of x [B, ...] against t, one plane per image: overlap.overlap_loss_host with cfg's fp / fn /
    focal / smooth (an `overlap.OverlapLoss`; the kernel takes them as fp32) on x * mask (mask None: the disc form) — 0-dim device
    fp32; want_planes: -> (loss, per-plane losses [B]).  With dx the call adds the gradient of (*w_dev) * loss into dx IN PLACE
    (w_dev: device fp32 scalar, read by the kernel)."""
    _chk(x, "x"); _chk(t, "t"); _chk(mask, "mask"); _chk(dx, "dx"); _chk(w_dev, "w_dev")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError("overlap_loss: logits [B, ..., H, W], got shape %s" % (tuple(x.shape),))
    n, B = x.numel(), int(x.shape[0])
    for name, v in (("t", t), ("mask", mask), ("dx", dx)):
        if v is not None and v.numel() != n:
            raise ValueError("overlap_loss: %s has %d elements, x has %d" % (name, v.numel(), n))
    if dx is not None and w_dev is None:
        raise ValueError("overlap_loss: dx needs the device weight w_dev")
    L = lib()
    nbytes = L.query("wtpse_overlap_loss_ws", B, n // B)
    if nbytes <= 0:
        raise ValueError("overlap_loss: unsupported size %s" % (tuple(x.shape),))
    # an amax table that describes the region loss's gradient alone no longer bounds dx
    _amax_stale(dx)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    planes = torch.empty((B,), dtype=torch.float32, device=x.device) if want_planes else None
    ws = workspace("overlap_loss", (nbytes + 3) // 4, x.device)
    L.call("wtpse_overlap_loss", ptr(x), ptr(mask), ptr(t), ptr(w_dev), B, n // B, float(cfg.fp), float(cfg.fn), float(cfg.focal),
           float(cfg.smooth), ptr(ws), ptr(planes), ptr(loss), ptr(dx), stream_ptr())
    return (loss, planes) if want_planes else loss


def lovasz_loss(x, t, w_dev, mask=None, dx=None, want_planes=False, want_ranks=False):
    """-> the unweighted Lovász hinge loss of x [B, ...] against t, one plane per image: lovasz.lovasz_loss_host, the pixels with
    mask == 0 taken out of the set (mask None: the disc form) — 0-dim device fp32; want_planes: also the per-plane losses [B];
    want_ranks: also every pixel's place in its plane's order (int32 of x's shape, lovasz.lovasz_ranks_host), in that order behind
    the loss.  With dx the call adds the gradient of (*w_dev) * loss into dx IN PLACE (w_dev: device fp32 scalar, read by the kernel)."""
    _chk(x, "x"); _chk(t, "t"); _chk(mask, "mask"); _chk(dx, "dx"); _chk(w_dev, "w_dev")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError("lovasz_loss: logits [B, ..., H, W], got shape %s" % (tuple(x.shape),))
    n, B = x.numel(), int(x.shape[0])
    for name, v in (("t", t), ("mask", mask), ("dx", dx)):
        if v is not None and v.numel() != n:
            raise ValueError("lovasz_loss: %s has %d elements, x has %d" % (name, v.numel(), n))
    if dx is not None and w_dev is None:
        raise ValueError("lovasz_loss: dx needs the device weight w_dev")
    L = lib()
    nbytes = L.query("wtpse_lovasz_loss_ws", B, n // B)
    if nbytes <= 0:
        raise ValueError("lovasz_loss: unsupported size %s" % (tuple(x.shape),))
    # an amax table that describes the region loss's gradient alone no longer bounds dx
    _amax_stale(dx)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    planes = torch.empty((B,), dtype=torch.float32, device=x.device) if want_planes else None
    ranks = torch.empty(x.shape, dtype=torch.int32, device=x.device) if want_ranks else None
    ws = workspace("lovasz_loss", (nbytes + 3) // 4, x.device)
    L.call("wtpse_lovasz_loss", ptr(x), ptr(mask), ptr(t), ptr(w_dev), B, n // B, ptr(ws), ptr(planes), ptr(ranks), ptr(loss), ptr(dx),
           stream_ptr())
    out = (loss,) + ((planes,) if want_planes else ()) + ((ranks,) if want_ranks else ())
    return out if len(out) > 1 else loss


def roi(image, logit):
    B, C, H, W = image.shape
    out = torch.empty_like(image)
    od = torch.empty_like(logit)
    lib().call("wtpse_roi", ptr(image), ptr(logit), ptr(out), ptr(od), B, C, H * W, stream_ptr())
    return out, od


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, step_dev=None):
    """Step number t = step + *step_dev (step_dev: device int32 count of completed steps, or None)."""
    _amax_stale(p)
    lib().call("wtpse_adam", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
               int(step), ptr(step_dev), stream_ptr())


def adam_step_dev(p, g, m, v, lr_dev, beta1, beta2, eps, step, step_dev=None, hold=None):
    """adam_step with the learning rate in device memory (lr_dev: one fp32) and an optional hold flag (device int32: non-zero =
    the launch changes nothing)."""
    _amax_stale(p)
    lib().call("wtpse_adam_dev", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(lr_dev), float(beta1), float(beta2), float(eps),
               int(step), ptr(step_dev), ptr(hold), stream_ptr())


def adam_index(p, g, m, v, idx, lr_dev, beta1, beta2, eps, step, step_dev=None, hold=None):
    """adam_step_dev on the elements p[idx] of a flat buffer alone (idx: device int32 [n] of distinct positions, checked by whoever
    built it), with COMPACT moments m, v [n]: bitwise adam_step_dev on those elements, everything else of p untouched."""
    _chk(p, "p"); _chk(g, "g"); _chk(m, "m"); _chk(v, "v")
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 1 and idx.numel() > 0):
        raise ValueError("adam_index: idx must be a non-empty contiguous int32 vector in device memory")
    n = idx.numel()
    if p.numel() != g.numel() or m.numel() != n or v.numel() != n:
        raise ValueError("adam_index: p and g must have one length, m and v that of idx (got %d, %d, %d, %d for %d indices)"
                         % (p.numel(), g.numel(), m.numel(), v.numel(), n))
    _amax_stale(p)
    lib().call("wtpse_adam_index", ptr(p), ptr(g), ptr(m), ptr(v), ptr(idx), n, ptr(lr_dev), float(beta1), float(beta2), float(eps),
               int(step), ptr(step_dev), ptr(hold), stream_ptr())


def entropy_loss(x, mask=None, margin=float("inf"), reweight=False, want_planes=False, want_grad=True):
    """The entropy objective of x [B, ..., H, W], one plane per image: tent.tent_loss_host on x * mask (mask None: the disc form)
    -> (loss, dx): the 0-dim device fp32 loss and its gradient wrt x, WRITTEN into a fresh tensor (every element; an unselected
    plane's are +0.0); want_planes: -> (loss, dx, planes [B] fp32, selected [B] int32).  want_grad=False: dx is None, nothing but
    the value is computed.  margin in nats (inf: every plane with a non-empty mask is selected), reweight: EATA's exp(margin - H_b)."""
    _chk(x, "x"); _chk(mask, "mask")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError("entropy_loss: logits [B, ..., H, W], got shape %s" % (tuple(x.shape),))
    n, B = x.numel(), int(x.shape[0])
    if mask is not None and mask.numel() != n:
        raise ValueError("entropy_loss: mask has %d elements, x has %d" % (mask.numel(), n))
    margin = float(margin)
    if not margin > 0.0:
        raise ValueError("entropy_loss: margin must be positive (nats; inf: no filter), got %r" % (margin,))
    L = lib()
    nbytes = L.query("wtpse_entropy_loss_ws", B, n // B)
    if nbytes <= 0:
        raise ValueError("entropy_loss: unsupported size %s" % (tuple(x.shape),))
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if want_grad else None
    planes = torch.empty((B,), dtype=torch.float32, device=x.device) if want_planes else None
    selected = torch.empty((B,), dtype=torch.int32, device=x.device) if want_planes else None
    ws = workspace("entropy_loss", (nbytes + 3) // 4, x.device)
    L.call("wtpse_entropy_loss", ptr(x), ptr(mask), B, n // B, margin, int(bool(reweight)), ptr(ws), ptr(planes), ptr(selected),
           ptr(loss), ptr(dx), stream_ptr())
    return (loss, dx, planes, selected) if want_planes else (loss, dx)


def loss_log_code(k):
    """wtpse_loss_log's check_n for "NaN-test the first k scalars" (the table of include/wtpse_hip.h)."""
    if not 0 <= k <= 6:
        raise ValueError("loss_log: the NaN test covers the first 0 to 6 scalars of a call, got %d" % k)
    return (0, 1, 17, 3, 19, 51, 115)[k]


def loss_log(scalars, acc, offset, check_n, flag, step_dev):
    """acc[offset + j] += scalars[j] (up to six 0-dim fp32 device tensors; acc: device float64) and the reference's NaN test on the
    first scalars into flag (device int32 [2]): check_n is the code of their count, `loss_log_code(k)`; see wtpse_loss_log in
    include/wtpse_hip.h."""
    if not 1 <= len(scalars) <= 6 or offset + len(scalars) > acc.numel():
        raise ValueError("loss_log: %d scalars at offset %d of an accumulator of %d" % (len(scalars), offset, acc.numel()))
    s = [ptr(t) for t in scalars] + [0] * (6 - len(scalars))
    lib().call("wtpse_loss_log", *s, acc.data_ptr() + 8 * int(offset), int(check_n), ptr(flag), ptr(step_dev), stream_ptr())


def avg_step(avgs, params, count, gate=None, hold=None):
    """One iterate into the running means (wtpse_avg_step): up to four (mean, iterate) pairs of flat fp32 tensors in ONE call;
    count: device int32 (iterates folded so far; bumped behind the fold); gate / hold: optional device int32 — *gate == 0 or
    *hold != 0 leaves means and count untouched."""
    if len(avgs) != len(params) or not 1 <= len(avgs) <= 4:
        raise ValueError("avg_step: one to four (mean, iterate) pairs, got %d / %d" % (len(avgs), len(params)))
    args = []
    for a, p in zip(avgs, params):
        _chk(a, "mean"); _chk(p, "iterate")
        if a.numel() != p.numel():
            raise ValueError("avg_step: a mean of %d elements for an iterate of %d" % (a.numel(), p.numel()))
        args += [ptr(a), ptr(p), a.numel()]
    args += [0, 0, 0] * (4 - len(avgs))
    lib().call("wtpse_avg_step", *args, ptr(count), ptr(gate), ptr(hold), stream_ptr())


def avg_merge(acc, seg, n_acc, n_seg):
    """acc (the mean of n_acc iterates) <- the mean of the n_acc + n_seg iterates that acc and seg (the mean of n_seg) cover, in
    place (wtpse_avg_merge); n_acc == 0 copies.  -> acc."""
    _chk(acc, "acc"); _chk(seg, "seg")
    if acc.numel() != seg.numel():
        raise ValueError("avg_merge: %d elements against %d" % (acc.numel(), seg.numel()))
    _amax_stale(acc)
    lib().call("wtpse_avg_merge", ptr(acc), ptr(seg), acc.numel(), int(n_acc), int(n_seg), stream_ptr())
    return acc


# ----------------------------------------------------------------------------------------------- validation back half
def _chk_dev(t, name, dtype):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.dim() == 4 and t.shape[1] == 1):
        raise ValueError("%s must be a contiguous [B,1,h,w] %s tensor in device memory (got %s, %s, %s)"
                         % (name, dtype, tuple(t.shape), t.device, t.dtype))


def postprocess_masks(logits, threshold=0.75):
    """utils.postprocessing on the device: [B,1,h,w] fp32 logits -> uint8 [B,1,h,w] = largest 8-connected component of
    sigmoid > threshold, holes filled (bit for bit validate.postprocess)."""
    _chk_dev(logits, "logits", torch.float32)
    B, _, h, w = logits.shape
    L = lib()
    words = L.query("wtpse_postprocess_ws", B, h, w)
    if words <= 0:
        raise ValueError("postprocess_masks: unsupported size %s (1 <= h, w <= 4096)" % (tuple(logits.shape),))
    out = torch.empty((B, 1, h, w), dtype=torch.uint8, device=logits.device)
    ws = workspace("postprocess", words, logits.device)
    L.call("wtpse_postprocess", ptr(logits), ptr(out), ptr(ws), float(threshold), B, h, w, stream_ptr())
    return out


SEG_FIELDS = ("inter", "n_pred", "n_label", "surf_pred", "surf_label", "d2_lo", "d2_hi", "asd_sum")


def seg_metrics(mask, label):
    """Raw per-image records [B,8] int64 (fields SEG_FIELDS; the last one holds float64 bits) of a uint8 mask against an fp32
    label (nonzero = object), both [B,1,h,w] on the device.  validate.device_metrics finishes them."""
    _chk_dev(mask, "mask", torch.uint8)
    _chk_dev(label, "label", torch.float32)
    if mask.shape != label.shape or mask.device != label.device:
        raise ValueError("mask %s and label %s differ in shape or device" % (tuple(mask.shape), tuple(label.shape)))
    B, _, h, w = mask.shape
    L = lib()
    words = L.query("wtpse_seg_metrics_ws", B, h, w)
    if words <= 0:
        raise ValueError("seg_metrics: unsupported size %s (1 <= h, w <= 4096)" % (tuple(mask.shape),))
    rec = torch.empty((B, 8), dtype=torch.int64, device=mask.device)
    ws = workspace("seg_metrics", words, mask.device)
    L.call("wtpse_seg_metrics", ptr(mask), ptr(label), ptr(rec), ptr(ws), B, h, w, stream_ptr())
    return rec


# ----------------------------------------------------------------------------------------------- test run
def overlay(img, pred_od, pred_oc, gt_od, gt_oc):
    """The pictures of the reference's test program on the device (csrc/overlay.hip; test_run.overlay_host byte for byte):
    img [B,3,h,w] fp32 (normalised, at the label size), pred_od / pred_oc [B,1,h,w] uint8 (postprocess_masks), gt_od / gt_oc
    [B,1,h,w] uint8 labels 0 / 1 -> (original, overlay), each uint8 [B,h,w,3].  gt_od = gt_oc = None: no ground truth
    (wtpse_overlay_pred) — the pictures an all-zero ground truth gives, without its largest-component stage."""
    _chk(img, "img")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("img must be [B,3,h,w] (got %s)" % (tuple(img.shape),))
    B, _, h, w = img.shape
    if (gt_od is None) != (gt_oc is None):
        raise ValueError("gt_od and gt_oc are given together or both None")
    masks = ((pred_od, "pred_od"), (pred_oc, "pred_oc"))
    if gt_od is not None:
        masks += ((gt_od, "gt_od"), (gt_oc, "gt_oc"))
    for t, name in masks:
        _chk_dev(t, name, torch.uint8)
        if tuple(t.shape) != (B, 1, h, w) or t.device != img.device:
            raise ValueError("%s %s (%s) does not match img %s (%s)" % (name, tuple(t.shape), t.device, tuple(img.shape), img.device))
    L = lib()
    words = L.query("wtpse_overlay_ws" if gt_od is not None else "wtpse_overlay_pred_ws", B, h, w)
    if words < 0 or (words == 0 and gt_od is not None):
        raise ValueError("overlay: unsupported size %s (2 <= h, w <= 4096)" % (tuple(img.shape),))
    original = torch.empty((B, h, w, 3), dtype=torch.uint8, device=img.device)
    over = torch.empty((B, h, w, 3), dtype=torch.uint8, device=img.device)
    if gt_od is None:
        L.call("wtpse_overlay_pred", ptr(img), ptr(pred_od), ptr(pred_oc), ptr(original), ptr(over), B, h, w, stream_ptr())
        return original, over
    ws = workspace("overlay", words, img.device)
    L.call("wtpse_overlay", ptr(img), ptr(pred_od), ptr(pred_oc), ptr(gt_od), ptr(gt_oc), ptr(original), ptr(over), ptr(ws), B, h, w,
           stream_ptr())
    return original, over


def label_thresholds(mask):
    """Grey-level masks uint8 [B,1,h,w] -> (original_od, original_oc) fp32 [B,1,h,w]: 1 where the byte is <= 200 / <= 50
    (fundus_dataloader.py:112-134)."""
    _chk_dev(mask, "mask", torch.uint8)
    od = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    oc = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    lib().call("wtpse_label_thresholds", ptr(mask), ptr(od), ptr(oc), mask.numel(), stream_ptr())
    return od, oc


# ----------------------------------------------------------------------------------------------- segmenting unlabelled images
def image_finish(img_u8):
    """[N,S,S,3] uint8 on the device -> [N,3,S,S] fp32 = img / 127.5 - 1 (two roundings): wtpse_input_finish's image, no mask."""
    t = img_u8
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 4 and t.shape[3] == 3 and t.shape[1] == t.shape[2]):
        raise ValueError("img_u8 must be a contiguous [N,S,S,3] uint8 tensor in device memory (got %s, %s, %s)"
                         % (tuple(t.shape), t.device, t.dtype))
    N, S = t.shape[0], t.shape[1]
    image = torch.empty((N, 3, S, S), dtype=torch.float32, device=t.device)
    lib().call("wtpse_image_finish", ptr(t), ptr(image), N, S, stream_ptr())
    return image


def label_map(disc, cup):
    """Two uint8 masks [B,1,h,w] (nonzero = object) -> the grey-level label uint8 [B,1,h,w]: 0 where cup, else 128 where disc, else
    255 (segment.label_map_host byte for byte; label_thresholds reads it back)."""
    _chk_dev(disc, "disc", torch.uint8)
    _chk_dev(cup, "cup", torch.uint8)
    if disc.shape != cup.shape or disc.device != cup.device:
        raise ValueError("disc %s and cup %s differ in shape or device" % (tuple(disc.shape), tuple(cup.shape)))
    out = torch.empty(disc.shape, dtype=torch.uint8, device=disc.device)
    lib().call("wtpse_label_map", ptr(disc), ptr(cup), ptr(out), disc.numel(), stream_ptr())
    return out


GEOMETRY_FIELDS = ("area", "top", "bottom", "left", "right", "sum_r", "sum_c", "reserved")


def mask_geometry(mask):
    """uint8 masks [B,1,h,w] on the device -> records [B,8] int64 (fields GEOMETRY_FIELDS) over the nonzero pixels; an empty mask:
    (0, h, -1, w, -1, 0, 0, 0).  segment.mask_geometry_host exactly; segment.measure finishes a pair of them."""
    _chk_dev(mask, "mask", torch.uint8)
    B, _, h, w = mask.shape
    if not (1 <= B < 8192 and 1 <= h <= 4096 and 1 <= w <= 4096):
        raise ValueError("mask_geometry: unsupported size %s (1 <= h, w <= 4096)" % (tuple(mask.shape),))
    rec = torch.empty((B, 8), dtype=torch.int64, device=mask.device)
    lib().call("wtpse_mask_geometry", ptr(mask), ptr(rec), B, h, w, stream_ptr())
    return rec


# ----------------------------------------------------------------------------------------------- optic-disc morphometry
PROFILE_FIELDS = ("disc_r2", "cup_r2", "disc_n", "cup_n")
_SECTOR_TABLES = {}


def onh_profile(disc, cup, geom_disc, N=24):
    """Two uint8 masks [B,1,h,w] (nonzero = object) and the disc's mask_geometry records [B,8] int64, all on one device ->
    (profile [B,N,4] int32 holding uint32 bits, fields PROFILE_FIELDS per angular sector around the disc's centroid; moments [B,2,4]
    int64 = per mask (sum y^2, sum x^2, sum x y, .) with the centre 2 cy / 2 cx in the disc's / the cup's fourth slot).
    morphometry.profile_host exactly (view the profile as uint32 on the host); morphometry.finish finishes a row.  The sector table
    (morphometry.sector_table) is kept on the device per (device, N)."""
    from . import morphometry as M
    _chk_dev(disc, "disc", torch.uint8)
    _chk_dev(cup, "cup", torch.uint8)
    N = M.check_sectors(N)
    B, _, h, w = disc.shape
    if disc.shape != cup.shape or disc.device != cup.device:
        raise ValueError("disc %s and cup %s differ in shape or device" % (tuple(disc.shape), tuple(cup.shape)))
    g = geom_disc
    if not (torch.is_tensor(g) and g.is_cuda and g.dtype == torch.int64 and g.is_contiguous() and tuple(g.shape) == (B, 8)
            and g.device == disc.device):
        raise ValueError("geom_disc must be the contiguous [%d,8] int64 records of the discs on %s (got %s, %s, %s)"
                         % (B, disc.device, tuple(g.shape) if torch.is_tensor(g) else type(g), getattr(g, "device", None),
                            getattr(g, "dtype", None)))
    if not (1 <= B < 8192 and 1 <= h <= 4096 and 1 <= w <= 4096):
        raise ValueError("onh_profile: unsupported size %s (B < 8192, 1 <= h, w <= 4096)" % (tuple(disc.shape),))
    key = (disc.device, N)
    table = _SECTOR_TABLES.get(key)
    if table is None:
        table = _SECTOR_TABLES[key] = torch.from_numpy(M.sector_table(N)).to(disc.device)
    profile = torch.empty((B, N, 4), dtype=torch.int32, device=disc.device)
    moments = torch.empty((B, 2, 4), dtype=torch.int64, device=disc.device)
    lib().call("wtpse_onh_profile", ptr(disc), ptr(cup), ptr(g), ptr(table), ptr(profile), ptr(moments), N, B, h, w, stream_ptr())
    return profile, moments


# ----------------------------------------------------------------------------------------------- calibration against labels
CAL_BINS = 1024
CAL_REC = 2 * (CAL_BINS + 1) * 2 + 4


def calibration_hist(prob, spread, label, region=None, threshold=0.75):
    """prob, label [B,1,h,w] fp32 (label: nonzero = object), spread the same or None (every spread 0), region [B,1,h,w] uint8 or None
    (every pixel), all on one device -> records [B, CAL_REC] int32 holding uint32 bits: hist_p [CAL_BINS + 1, 2], hist_s
    [CAL_BINS + 1, 2], tail [4] (include/wtpse_hip.h).  calibration.hist_host exactly (view the records as uint32 on the host);
    calibration.split_record names the parts."""
    _chk_dev(prob, "prob", torch.float32)
    _chk_dev(label, "label", torch.float32)
    for t, name, dtype in ((spread, "spread", torch.float32), (region, "region", torch.uint8)):
        if t is not None:
            _chk_dev(t, name, dtype)
    for t, name in ((label, "label"), (spread, "spread"), (region, "region")):
        if t is not None and (t.shape != prob.shape or t.device != prob.device):
            raise ValueError("prob %s (%s) and %s %s (%s) differ in shape or device" % (tuple(prob.shape), prob.device, name, tuple(t.shape), t.device))
    B, _, h, w = prob.shape
    if not (1 <= B < 8192 and 1 <= h <= 4096 and 1 <= w <= 4096):
        raise ValueError("calibration_hist: unsupported size %s (B < 8192, 1 <= h, w <= 4096)" % (tuple(prob.shape),))
    rec = torch.empty((B, CAL_REC), dtype=torch.int32, device=prob.device)
    lib().call("wtpse_calibration_hist", ptr(prob), ptr(spread) if spread is not None else 0, ptr(label),
               ptr(region) if region is not None else 0, float(threshold), ptr(rec), B, h, w, stream_ptr())
    return rec


# ----------------------------------------------------------------------------------------------- test-time views
_VIEW_CODES = {}


def _view_codes(codes):
    """The host int array wtpse_dihedral_views / wtpse_views_merge read their codes from, kept per code tuple (a recorded launch
    plan holds the pointer)."""
    import ctypes
    key = tuple(int(c) for c in codes)
    arr = _VIEW_CODES.get(key)
    if arr is None:
        arr = _VIEW_CODES[key] = (ctypes.c_int * max(len(key), 1))(*key)
    return key, ctypes.addressof(arr)


def dihedral_views(x, codes):
    """x [B,C,S,S] -> [V,B,C,S,S]: plane (b, c) of view v is views.view_host(x[b, c], codes[v]), bit for bit (csrc/views.hip).  The
    result is freshly allocated on every call: amax_of keeps its table on the tensor object it is given, and a reused buffer
    would hand the U-Nets the x2h scale of an earlier batch."""
    _chk(x, "x")
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError("dihedral_views: x must be [B,C,S,S] with square planes (got %s)" % (tuple(x.shape),))
    B, C, S, _ = x.shape
    key, cptr = _view_codes(codes)
    out = torch.empty((len(key), B, C, S, S), dtype=torch.float32, device=x.device)
    lib().call("wtpse_dihedral_views", ptr(x), ptr(out), cptr, len(key), B * C, S, stream_ptr())
    return out


def views_merge(logits, codes, threshold=0.75, want_logits=True, want_mean_logit=True):
    """logits [V,B,K,S,S], each view's maps in its own frame -> (mean, std [B,1,S,S] fp32, votes [B,1,S,S] uint8, logits
    [B,V*K,S,S] un-viewed with sample index v*K + k or None, mean_logit [B,1,S,S] or None): one launch (csrc/views.hip;
    views.merge_host is its specification).  Every output is freshly allocated."""
    _chk(logits, "logits")
    if logits.dim() != 5 or logits.shape[3] != logits.shape[4]:
        raise ValueError("views_merge: logits must be [V,B,K,S,S] with square planes (got %s)" % (tuple(logits.shape),))
    V, B, K, S, _ = logits.shape
    key, cptr = _view_codes(codes)
    if len(key) != V:
        raise ValueError("views_merge: %d codes for %d views" % (len(key), V))
    dev = logits.device
    mean = torch.empty((B, 1, S, S), dtype=torch.float32, device=dev)
    std = torch.empty((B, 1, S, S), dtype=torch.float32, device=dev)
    votes = torch.empty((B, 1, S, S), dtype=torch.uint8, device=dev)
    out = torch.empty((B, V * K, S, S), dtype=torch.float32, device=dev) if want_logits else None
    mean_logit = torch.empty((B, 1, S, S), dtype=torch.float32, device=dev) if want_mean_logit else None
    lib().call("wtpse_views_merge", ptr(logits), cptr, V, B, K, S, float(threshold), ptr(out), ptr(mean), ptr(std), ptr(votes),
               ptr(mean_logit), stream_ptr())
    return mean, std, votes, out, mean_logit


# ----------------------------------------------------------------------------------------------- whole fundus photographs
def _chk_u8(t, name, dims):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == dims):
        raise ValueError("%s must be a contiguous %d-d uint8 tensor in device memory (got %s)"
                         % (name, dims, (tuple(t.shape), t.device, t.dtype, t.is_contiguous()) if isinstance(t, torch.Tensor) else type(t)))


def locate_cells(img, c, t):
    """[N,H,W,3] uint8 on the device -> int64 [N, ceil(H/c), ceil(W/c), 2] = per c x c cell (n, s) over its pixels with
    max(R,G,B) >= t: their count and the sum of 77 R + 150 G + 29 B (csrc/locate.hip; locate.cells_host bit for bit)."""
    _chk_u8(img, "img", 4)
    N, H, W, C = img.shape
    c, t = int(c), int(t)
    if C != 3 or not (1 <= N <= 65535 and 1 <= H <= 65536 and 1 <= W <= 65536):
        raise ValueError("locate_cells: img must be [N,H,W,3] with 1 <= H, W <= 65536 (got %s)" % (tuple(img.shape),))
    if not 2 <= c <= 256 or not 0 <= t <= 255:
        raise ValueError("locate_cells: the cell side must lie in 2..256 and the threshold in 0..255 (got %r, %r)" % (c, t))
    out = torch.empty((N, -(-H // c), -(-W // c), 2), dtype=torch.int64, device=img.device)
    lib().call("wtpse_locate_cells", ptr(img), ptr(out), N, H, W, c, t, stream_ptr())
    return out


GRAD_REC = 276


def gradability_record(img, t=24, sat=250):
    """[N,H,W,3] (or [H,W,3]) uint8 on the device -> int64 [N, GRAD_REC] (N = 1 for one picture): per picture the luma histogram,
    channel sums, saturation counts, area and bounding box of its field (max(R,G,B) >= t) and the Laplacian / gradient energies of
    the green channel at the dilations 1, 2, 4 (csrc/gradability.hip; gradability.record_host bit for bit, gradability.split_record
    names the parts)."""
    if isinstance(img, torch.Tensor) and img.dim() == 3:
        img = img[None]
    _chk_u8(img, "img", 4)
    N, H, W, C = img.shape
    t, sat = int(t), int(sat)
    if C != 3 or not (1 <= N <= 65535 and 1 <= H <= 65536 and 1 <= W <= 65536):
        raise ValueError("gradability_record: img must be [N,H,W,3] with 1 <= H, W <= 65536 (got %s)" % (tuple(img.shape),))
    if not 0 <= t <= 255 or not 1 <= sat <= 255:
        raise ValueError("gradability_record: the threshold must lie in 0..255 and sat in 1..255 (got %r, %r)" % (t, sat))
    rec = torch.empty((N, GRAD_REC), dtype=torch.int64, device=img.device)
    lib().call("wtpse_gradability_record", ptr(img), ptr(rec), N, H, W, t, sat, stream_ptr())
    return rec


def crop_u8(img, boxes, side):
    """One [H,W,C] uint8 picture (C = 1 or 3) and boxes [M,2] int32 = (top, left), both on the device -> [M,side,side,C]: the boxes'
    pixels, 0 beyond the picture's borders (locate.crop_host bit for bit)."""
    _chk_u8(img, "img", 3)
    H, W, C = img.shape
    side = int(side)
    if not (boxes.is_cuda and boxes.device == img.device and boxes.dtype == torch.int32 and boxes.is_contiguous() and boxes.dim() == 2
            and boxes.shape[1] == 2 and 1 <= boxes.shape[0] <= 65535):
        raise ValueError("crop_u8: boxes must be a contiguous [M,2] int32 tensor on img's device (got %s, %s, %s)"
                         % (tuple(boxes.shape), boxes.device, boxes.dtype))
    if C not in (1, 3) or not (1 <= H <= 65536 and 1 <= W <= 65536 and 1 <= side <= 8192):
        raise ValueError("crop_u8: img must be [H,W,1 or 3] with 1 <= H, W <= 65536 and 1 <= side <= 8192 (got %s, %r)" % (tuple(img.shape), side))
    M = boxes.shape[0]
    out = torch.empty((M, side, side, C), dtype=torch.uint8, device=img.device)
    lib().call("wtpse_crop_u8", ptr(img), ptr(boxes), ptr(out), H, W, C, M, side, stream_ptr())
    return out


def paste_u8(canvas, patch, top, left):
    """canvas [H,W,C] uint8 on the device, IN PLACE: the patch [h,w,C] lands with its corner at (top, left), clipped at the canvas'
    borders; wholly outside changes nothing (locate.paste_host bit for bit).  -> canvas."""
    _chk_u8(canvas, "canvas", 3)
    _chk_u8(patch, "patch", 3)
    H, W, C = canvas.shape
    h, w = patch.shape[:2]
    top, left = int(top), int(left)
    if C not in (1, 3) or patch.shape[2] != C or patch.device != canvas.device or min(H, W, h, w) < 1 or max(H, W, h, w) > 65536:
        raise ValueError("paste_u8: canvas %s and patch %s must share C = 1 or 3 and a device, sides in 1..65536"
                         % (tuple(canvas.shape), tuple(patch.shape)))
    if max(abs(top), abs(left)) > 1 << 24:
        raise ValueError("paste_u8: |top|, |left| must not exceed 2^24 (got %r, %r)" % (top, left))
    lib().call("wtpse_paste_u8", ptr(canvas), ptr(patch), H, W, C, h, w, top, left, stream_ptr())
    return canvas


# ----------------------------------------------------------------------------------------------- input stages
def _chk_stage_batch(img, who, side_max, square=True):
    """What every input stage asks of its batch: a contiguous uint8 tensor in device memory, [N,S,S,3] (or [N,H,W,3] with
    square=False), 1 <= N <= 65535 (a grid dimension), sides 1 .. side_max.  who: the wrapper's name, for the message.
    -> (N, H, W)."""
    _chk_u8(img, "img", 4)
    N, H, W, C = (int(s) for s in img.shape)
    if C != 3 or (square and H != W) or not 1 <= N <= 65535 or not (1 <= H <= side_max and 1 <= W <= side_max):
        raise ValueError("%s: img must be [N,%s,3] with 1 <= N <= 65535 and sides in 1 .. %d (got %s)"
                         % (who, "S,S" if square else "H,W", side_max, tuple(img.shape)))
    return N, H, W


# ----------------------------------------------------------------------------------------------- amplitude mixing
_TWIDDLES = {}


def amplitude_mix(img, partner, lam, b, want_float=False):
    """[N,S,S,3] uint8 on the device, partner [N] int (-1: leave the row alone) and lam [N] float on the host, b = half width of the
    frequency window -> the batch with the amplitude of every row that has a partner moved towards its partner's (csrc/spectrum.hip;
    input_pipeline.amplitude_mix_host is the specification); with want_float also the unrounded fp32 values [N,S,S,3]."""
    from .input_pipeline.amplitude_mix import MIX_SIZES, check_mix_params, twiddle_table
    import numpy as np
    N, S, _ = _chk_stage_batch(img, "amplitude_mix", MIX_SIZES[-1])
    partner, lam, b = check_mix_params(partner, lam, b, N, S)
    nfloats = lib().query("wtpse_amix_workspace", N, S, b)
    if nfloats < 0:
        raise ValueError("amplitude_mix: a [%d,%d,%d,3] batch with b = %d needs more workspace than one call can take" % (N, S, S, b))
    dev = img.device
    tw = _TWIDDLES.get((str(dev), S))
    if tw is None:
        tw = _TWIDDLES[(str(dev), S)] = torch.from_numpy(twiddle_table(S)).to(dev)
    work = workspace("amix", nfloats, dev)
    dpartner = torch.from_numpy(partner.astype(np.int32)).to(dev, non_blocking=True)
    dlam = torch.from_numpy(lam.astype(np.float32)).to(dev, non_blocking=True)
    out = torch.empty_like(img)
    outf = torch.empty(img.shape, dtype=torch.float32, device=dev) if want_float else None
    lib().call("wtpse_amplitude_mix", ptr(img), ptr(dpartner), ptr(dlam), ptr(tw), ptr(out), ptr(outf), ptr(work), N, S, b, stream_ptr())
    return (out, outf) if want_float else out


# ----------------------------------------------------------------------------------------------- random appearance networks
_APPEARANCE_TABLES = {}


def appearance_axis(S, spacing, device):
    """The stage's axis table [S,5] int32 on `device` (input_pipeline.appearance_axis_table), kept per (S, spacing, device)."""
    from .input_pipeline.appearance import appearance_axis_table
    import numpy as np
    key = (int(S), int(spacing), str(device))
    t = _APPEARANCE_TABLES.get(key)
    if t is None:
        if len(_APPEARANCE_TABLES) >= 64:
            _APPEARANCE_TABLES.clear()
        t = _APPEARANCE_TABLES[key] = torch.from_numpy(appearance_axis_table(S, spacing).astype(np.int32)).to(device)
    return t


def appearance_nets(img, params, field, spacing):
    """[N,S,S,3] uint8 on the device, (params [N,389], field [N,G,G]) integers on the host (input_pipeline.draw_appearance) and the
    field's spacing -> the batch after the random appearance networks, a new tensor (csrc/appearance.hip: the nets tile by tile in
    LDS, then scaling and blend; input_pipeline.appearance_host is the specification, byte for byte).  The input is not written."""
    from .input_pipeline.appearance import APPEARANCE_MAX_SIZE, appearance_grid, check_appearance_params
    import numpy as np
    N, S, _ = _chk_stage_batch(img, "appearance_nets", APPEARANCE_MAX_SIZE)
    params, field = check_appearance_params(params, field, N, S, spacing)
    words = lib().query("wtpse_appearance_workspace", N, S)
    if words < 0:
        raise ValueError("appearance_nets: a [%d,%d,%d,3] batch needs more workspace than one call can take" % (N, S, S))
    dev = img.device
    axis = appearance_axis(S, spacing, dev)
    work = workspace("appearance", words, dev)
    # every table stays referenced until the launches are queued: a temporary's block would be handed to the next allocation
    # (C order whatever the caller's strides: a broadcast field keeps its stride order through astype)
    dparams = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev, non_blocking=True)
    dfield = torch.from_numpy(np.ascontiguousarray(field, dtype=np.int32)).to(dev, non_blocking=True)
    out = torch.empty_like(img)
    lib().call("wtpse_appearance_nets", ptr(img), ptr(dparams), ptr(work), N, S, stream_ptr())
    lib().call("wtpse_appearance_finish", ptr(img), ptr(dparams), ptr(dfield), ptr(axis), ptr(work), ptr(out), N, S,
               appearance_grid(S, spacing), stream_ptr())
    return out


# ----------------------------------------------------------------------------------------------- image quality
def image_quality(img, params, seed, pos, want_pos=False):
    """[N,S,S,3] uint8 on the device, params [N,13] integers on the host (a, c, beta, k, w[0..8] per sample:
    input_pipeline.draw_quality), the noise stream `seed` from position `pos` on -> the batch after focus, contrast, brightness and
    noise (csrc/quality.hip; input_pipeline.quality_host is the specification, byte for byte); with want_pos also the stream
    position behind the batch (S * S positions per sample with k > 0).  The input is not written."""
    from .input_pipeline.quality import QUALITY_MAX_SIZE, check_quality_params, quality_positions
    import numpy as np
    N, S, _ = _chk_stage_batch(img, "image_quality", QUALITY_MAX_SIZE)
    seed, pos = int(seed), int(pos)
    if not 0 <= seed < 1 << 64 or not 0 <= pos < 1 << 62:
        raise ValueError("image_quality: seed must lie in 0 .. 2^64 - 1 and pos in 0 .. 2^62 - 1 (got %r, %r)" % (seed, pos))
    params = check_quality_params(params, N)
    table, next_pos = quality_positions(params, S, pos)
    dev = img.device
    # every table stays referenced until the launches are queued: a temporary's block would be handed to the next allocation
    dparams = torch.from_numpy(params.astype(np.int32)).to(dev, non_blocking=True)
    dpos = torch.from_numpy(table.view(np.int64)).to(dev, non_blocking=True)
    sums = torch.empty(N, dtype=torch.int32, device=dev)
    out = torch.empty_like(img)
    lib().call("wtpse_quality_sums", ptr(img), ptr(sums), N, S, stream_ptr())
    lib().call("wtpse_quality_apply", ptr(img), ptr(dparams), ptr(sums), ptr(dpos), seed, ptr(out), N, S, stream_ptr())
    return (out, next_pos) if want_pos else out


# ----------------------------------------------------------------------------------------------- JPEG compression
def jpeg_roundtrip(img, mode, tables):
    """[N,S,S,3] uint8 on the device with S a multiple of 16, (mode [N], tables [N,2,64]) integers on the host
    (input_pipeline.draw_jpeg: mode 0 off, 1 = 4:4:4, 2 = 4:2:0; luma and chroma quantisation tables in natural order, 1 .. 255) ->
    the batch after baseline JPEG's round trip of the pixels, a new tensor (csrc/jpeg.hip; input_pipeline.jpeg_host is the
    specification, byte for byte, and is pinned to Pillow).  A batch whose modes are all 0 launches nothing and returns `img`
    itself.  The input is not written."""
    from .input_pipeline.jpeg import JPEG_MAX_SIZE, _check_jpeg_size, check_jpeg_params, jpeg_is_neutral, jpeg_reciprocals
    import numpy as np
    N, S, _ = _chk_stage_batch(img, "jpeg_roundtrip", JPEG_MAX_SIZE)
    _check_jpeg_size(S)
    mode, tables = check_jpeg_params(mode, tables, N)
    if jpeg_is_neutral(mode).all():
        return img
    if img.data_ptr() % 16:
        raise ValueError("jpeg_roundtrip: img must be 16-byte aligned (a view at an odd offset: clone it)")
    dev = img.device
    tables = np.where((mode != 0)[:, None, None], tables, 1)            # (the tables of a neutral row are not read: any reciprocal)
    # every table stays referenced until the launches are queued: a temporary's block would be handed to the next allocation
    dmode = torch.from_numpy(mode.astype(np.int32)).to(dev, non_blocking=True)
    dtab = torch.from_numpy(tables.astype(np.int32)).to(dev, non_blocking=True)
    drec = torch.from_numpy(jpeg_reciprocals(tables)).to(dev, non_blocking=True)
    chroma = torch.empty((N, 2, S // 2, S // 2), dtype=torch.uint8, device=dev) if (mode == 2).any() else None
    out = torch.empty_like(img)
    lib().call("wtpse_jpeg_roundtrip", ptr(img), ptr(dmode), ptr(dtab), ptr(drec), ptr(chroma), ptr(out), N, S, stream_ptr())
    return out


# ----------------------------------------------------------------------------------------------- CLAHE preprocessing
_CLAHE_TABLES = {}


def clahe_tables(H, W, clahe, device):
    """The stage's two axis tables on `device` (input_pipeline.clahe_device_tables), kept per (H, W, tiles, device)."""
    from .input_pipeline.clahe import clahe_device_tables
    key = (int(H), int(W), clahe.tiles, str(device))
    t = _CLAHE_TABLES.get(key)
    if t is None:
        if len(_CLAHE_TABLES) >= 64:
            _CLAHE_TABLES.clear()
        t = _CLAHE_TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in clahe_device_tables(H, W, clahe))
    return t


def clahe(img, clahe, want_luts=False):
    """[N,H,W,3] uint8 on the device and an input_pipeline.Clahe -> the equalised batch, a new tensor (csrc/clahe.hip: tile
    histograms, clipped LUTs, bilinear blend; input_pipeline.clahe_host is the specification, byte for byte); with want_luts also
    the tile LUTs [N,P,ty,tx,256] uint8.  The input is not written.  No draws: the same bytes on every call."""
    from .input_pipeline.clahe import CLAHE_MAX_SIDE, check_clahe
    N, H, W = _chk_stage_batch(img, "clahe", CLAHE_MAX_SIDE, square=False)
    check_clahe(clahe, H, W)
    (ty, tx), P, dev = clahe.tiles, clahe.planes, img.device
    rows, cols, bands = clahe_tables(H, W, clahe, dev)
    hist = torch.empty((N, P, ty, tx, 256), dtype=torch.int32, device=dev)
    luts = torch.empty((N, P, ty, tx, 256), dtype=torch.uint8, device=dev)
    out = torch.empty_like(img)
    st = stream_ptr()
    lib().call("wtpse_clahe_hist", ptr(img), ptr(hist), N, H, W, ty, tx, clahe.floor, P, st)
    lib().call("wtpse_clahe_lut", ptr(hist), ptr(luts), N * P * ty * tx, clahe.clip_q8, st)
    lib().call("wtpse_clahe_apply", ptr(img), ptr(luts), ptr(rows), ptr(cols), ptr(bands), ptr(out), N, H, W, ty, tx, clahe.floor, P, st)
    return (out, luts) if want_luts else out
