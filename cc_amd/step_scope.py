"""The process-wide state a training step switches on, and the one place that switches it.

A step runs with a dozen module-level variables of cc_amd/tape.py, cc_amd/ops.py and cc_amd/loss_functions.py set; their owners
define and read them, `StepScope` is the only code that assigns them.  Outside a scope they are IDLE:

    tape.BN_COUNTERS, tape.NET_DONE, tape.NET_MARK     None
    ops.grad_sinks                                     {}
    ops.wgrad_queue.enabled                            False, and nothing parked in ops.wgrad_queue / ops.wgrad_reduces
    ops.packs.valid, ops.packs.recording               False
    LF.scalar_pool.buf                                 None
    LF.head_grads.active                               False, LF.head_grads.acc empty
    LF.step_nan_flags, LF.forward_stream               None
(LF.pyramid_cache is emptied on entry: the frames' pyramids of one step are nobody else's.  What a step leaves in it stays until
the next entry or the owner's clear().)

Leaving the scope restores all of it on every path.  A normal exit launches the weight-gradient work that is still parked
(ops.wgrad_queue.flush(): every stream's queue on its stream, this stream's reduce table behind it) and closes the weight images by
their protocol; an exception drops the parked work instead -- its operands belong to the failed step and no fork / join is in place
for the side streams -- and invalidates the images.

    with StepScope(device, sinks=opt.sinks, bn_counters=counters, nan_flags=flags, images="per_network") as scope:
        ...                                   # the step's own opening launches
        with scope.loss_phase():              # scalar pool + the shared head-gradient accumulators
            out = cc_forward(...)
            g = torch.autograd.grad(...)
        scope.park_weight_gradients()         # from here on same-shaped weight gradients gather into group launches
        with scope.network_hooks(done, mark): # tape.NET_DONE / NET_MARK for this backward call
            torch.autograd.backward(...)

Every argument is optional: what is not given stays idle (a forward-only validation pass names its flag list, a kernel test
nothing at all)."""
import contextlib

from . import config, loss_functions as LF, ops, tape

_open = None        # the scope the process is in: the state is global, so a second one cannot be entered inside it


class StepScope:
    """images: the weight-image protocol of ops.PackRegistry --
         "per_network"  begin_step() on entry (no launch when the previous step's tails rebuilt the images), end_step() on exit: the
                        images stay, they match the weights the step's own Adam segments wrote;
         "legacy"       prepack_all() on entry (one launch), invalidate() on exit: the optimizer runs behind the step;
         None           the images are not touched.
       After an exception the images are invalidated whichever protocol was begun."""

    def __init__(self, device=None, sinks=None, bn_counters=None, nan_flags=None, images=None):
        assert images in ("per_network", "legacy", None), images
        self.device, self.sinks, self.bn_counters, self.nan_flags, self.images = device, sinks, bn_counters, nan_flags, images

    def __enter__(self):
        global _open
        if _open is not None:
            raise RuntimeError("a StepScope is already open in this process: the state it owns is module-level")
        _open = self
        try:
            if self.bn_counters is not None:
                tape.BN_COUNTERS = self.bn_counters
                self.bn_counters.begin()
            LF.pyramid_cache.clear()
            if self.images == "per_network":
                ops.packs.begin_step()
            elif self.images == "legacy":
                ops.packs.prepack_all()        # every conv layer's [tap][c][m] weight images, one launch (weights changed in Adam)
            if self.sinks is not None:
                ops.grad_sinks = self.sinks
            LF.step_nan_flags = self.nan_flags
        except BaseException:
            self._restore(failed=True)
            raise
        return self

    def __exit__(self, exc_type, exc, tb):
        self._restore(failed=exc_type is not None)
        return False

    def _restore(self, failed):
        global _open
        tape.BN_COUNTERS = tape.NET_DONE = tape.NET_MARK = None
        LF.step_nan_flags = LF.forward_stream = None
        LF.head_grads.end()
        try:
            if not failed:
                ops.wgrad_queue.flush()
        finally:
            ops.wgrad_queue.drop()             # (nothing, behind a flush that returned)
            ops.wgrad_reduces.drop()
            ops.wgrad_queue.enabled = False
            LF.scalar_pool.end()
            ops.grad_sinks = {}
            if self.images == "per_network" and not failed:
                ops.packs.end_step()
            elif self.images is not None:
                ops.packs.invalidate()
            _open = None

    @contextlib.contextmanager
    def loss_phase(self):
        """Forward passes + losses + autograd.grad of the losses: the loss terms' zero-initialised scalars come out of ONE buffer
        (its fill is this phase's first launch, behind the step's opening ones; the scalars live to the end of the scope -- only with
        a `device`), and the terms' gradients of a shared network output meet in one accumulator (LF.head_grads: ONE backward pass
        per forward pass, so only in here)."""
        if self.device is not None:
            LF.scalar_pool.begin(self.device)
        LF.head_grads.begin()
        try:
            yield self
        finally:
            LF.head_grads.end()

    def park_weight_gradients(self):
        """behind the loss gradients: the networks' backward passes park same-shaped weight gradients and their second stages
        (ops._WgradQueue, ops._WgradReduces) until a stage's end flushes them"""
        ops.wgrad_queue.enabled = not config.debug.no_wgrad_queue

    @contextlib.contextmanager
    def network_hooks(self, done, mark=None):
        """tape.NET_DONE / tape.NET_MARK around the backward call of the per-network pipeline"""
        tape.NET_DONE, tape.NET_MARK = done, mark
        try:
            yield self
        finally:
            tape.NET_DONE = tape.NET_MARK = None


@contextlib.contextmanager
def forward_stream(stream):
    """LF.forward_stream = stream around the fused loss terms whose forward launches belong on a side stream (trainer.cc_forward:
    inside a step's scope or, forward-only, outside any)"""
    LF.forward_stream = stream
    try:
        yield
    finally:
        LF.forward_stream = None
