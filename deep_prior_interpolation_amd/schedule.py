"""The stream schedule of one iteration: which launches leave the main stream, where the main stream waits for them, and which gradients
were handed to autograd ahead of the stream that writes them.  One class, one instance (ops.sched)."""
import os

import torch

from . import _lib


class Schedule:
    """Side streams for weight gradients, branch streams for work off the critical path of the U-Net, and the joins of both.

    Side streams: dW of a layer depends only on (x, dy) and nothing downstream depends on it before the optimiser step, so it runs
    concurrently with the backward-data / BatchNorm-backward chain.  At the coarse levels of the U-Net a single kernel fills only part of
    the chip (tens to hundreds of workgroups), the pair fills more of it.

    Branch streams: work that is OFF the critical path of the U-Net runs beside it instead of in front of it.
      forward:  the ResPath of level l (skip branch: conv3x3 + conv1x1 + join + BatchNorm, mulresunet.py:99-113) depends only on the
                encoder output of its level, while its consumer — the level's concat — also waits for the whole deeper U;  the 1x1x1
                shortcut of a MultiRes block (HBM-bound) depends only on the block input, while the three 3x3x3 layers (matrix-bound)
                form the chain the block output waits for.
      backward: the ResPath's backward (BatchNorm backward, backward-data, two weight gradients) feeds the encoder block of its level,
                which the deeper U's backward reaches much later.
    An HBM-bound kernel beside a matrix-bound one costs ~20 % of its stand-alone time (tools/overlap_probe.py: 25->16 forward 0.80 ms +
    elementwise 0.43 ms = 0.89 ms side by side), and the coarse levels' launches leave most of the chip idle.
    Same kernels, same operands, same order per tensor: results are bit-identical to the serial schedule.

    The instance is process-wide ON PURPOSE, unlike ops.mode_scope (which is per host thread).  Autograd runs the backward of GPU nodes on
    its own device thread, not on the thread that called backward(); everything the backward of a node reads here (in_iteration, side_keep,
    deferred, branch_on()) was set by begin() on the calling thread and must be visible on that other thread, so it cannot be
    threading.local.  The price: one iteration at a time per process between begin() and finish()."""

    N_SIDE = 2          # weight gradients round-robin over this many side streams

    def __init__(self):
        env = os.environ.get
        # Weight gradients on the side streams.  Off by default: it pays when the iteration is GPU-bound (patches of >= 2^20 voxels, eager
        # loop: 40.7 -> 39.6 ms at 256x128x128) and costs host time when it is launch-bound (64^3 eager: 8.8 -> 11.3 ms).
        # Interpolator.optimize / bench.py switch it on by patch size (set_overlap); DPI_OVERLAP_WGRAD=0/1 forces it.
        self.overlap = env("DPI_OVERLAP_WGRAD", "0") == "1"
        # ... inside a hipGraph capture too (fork / join edges in the graph): the edges cost more than the overlap wins on the small patches
        # that are run as graphs (7.6 vs 7.9 ms per iteration at 64^3), it pays on GPU-bound ones (256x128x128: 34.2 ms eager with overlap,
        # 34.2 ms graph without, 33.8 ms graph with).
        self.overlap_in_graph = env("DPI_OVERLAP_IN_GRAPH", "0") == "1"
        # Where the main stream waits for the weight-gradient streams.  "node": at the end of every fused node's backward.  "step": once,
        # after the whole backward (finish(), before the optimiser step): the main chain never stalls behind a weight-gradient kernel, the
        # side streams drain their backlog under the BatchNorm-backward / up-sampling passes of the nodes that follow.
        # Only between begin() and finish() (the Interpolator's loops); a bare loss.backward() joins per node.
        self.join_at = env("DPI_JOIN_AT", "step")
        # Branch streams: only inside an iteration with the weight-gradient overlap on (patches >= 2^20 voxels, eager loop): branch_on().
        self.branch_streams = env("DPI_BRANCH", "1") == "1"
        # The 1x1x1 shortcut of a block on a branch stream.  0: OFF.  1: beside the block's first 3x3x3 layer — that layer (64->4, 67->4,
        # 25->8: few output channels) is itself at ~half the HBM bandwidth, the 1x1x1 layer beside it gains nothing (64->4 0.70 -> 1.05 ms
        # with the 0.35 ms shortcut beside it; 31.1-31.5 ms per iteration with, 30.6-30.8 without).  2: beside the SECOND and THIRD layer
        # (4->8, 8->13: matrix-bound, they read 4 / 8 channels), started once the first one has drained — measured +0.3 ms (29.7-30.1
        # against 29.3-29.5, profiles/r06/ab_fanin_shortcut.txt).
        self.branch_shortcut = int(env("DPI_BRANCH_SHORT", "0"))
        self.branch_skip = env("DPI_BRANCH_SKIP", "1") == "1"              # the ResPath half of a level join, forward
        self.branch_skip_bwd = env("DPI_BRANCH_SKIP_BWD", "1") == "1"      # ... and backward
        # ---- per-iteration state (cleared by _reset) ----
        self.in_iteration = False
        self.side_rr = 0                # next side stream of the round-robin; restarts in begin()
        self.side_used = set()          # side streams that have work since the last join
        # The tensors a side-stream launch reads were allocated on the main stream's pool; they are kept referenced here until the join
        # so that the caching allocator cannot hand their memory to a later main-stream tensor.
        self.side_keep = []
        self.branch_open = False
        # data_ptr of every gradient handed back to autograd BEFORE the stream that writes it has run (weight gradients on the side streams;
        # with the branch stream also the ResPath's BatchNorm gradients).  That is only sound if autograd's AccumulateGrad ADOPTS the tensor
        # as .grad — which needs .grad to be None (zero_grad with set_to_none=True), no hook, no second use of the parameter; anything else
        # makes it clone or add on the main stream, ahead of the producer.  finish(params) checks exactly that: every deferred tensor must
        # BE some parameter's .grad storage afterwards.
        self.deferred = []
        # ---- stream tables, per device, created lazily ----
        self._side_streams = {}         # device -> [N_SIDE streams]
        self._branch_streams = {}       # (device, kind) -> stream

    def set_overlap(self, on, in_graph=None):
        """Weight gradients on the side streams; in_graph: keep them there inside a hipGraph capture too.  A switch that is present in the
        environment (DPI_OVERLAP_WGRAD, DPI_OVERLAP_IN_GRAPH) wins."""
        if "DPI_OVERLAP_WGRAD" not in os.environ:
            self.overlap = bool(on)
        if in_graph is not None and "DPI_OVERLAP_IN_GRAPH" not in os.environ:
            self.overlap_in_graph = bool(in_graph)

    def _reset(self):
        self.in_iteration = False
        self.side_used.clear()
        del self.side_keep[:]
        del self.deferred[:]
        self.branch_open = False

    def begin(self):
        """Top of every iteration (eager or captured): the weight-gradient launches are dealt to the side streams from stream 0 again, so
        the kernel-to-stream assignment is the same in every iteration and every run."""
        self.side_rr = 0
        self.in_iteration = True
        del self.deferred[:]

    def abort(self):
        """An iteration raised between begin() and finish(): join every stream and forget the per-iteration state, so that a later bare
        loss.backward() joins per node again instead of believing it is still inside an Interpolator iteration."""
        try:
            if torch.cuda.is_available():
                self.join_side(final=True)
                self.join_branch()
        finally:
            self._reset()

    def finish(self, params=None):
        """After loss.backward(), before the optimiser step: every weight gradient launched on a side stream (and everything the branch
        stream still runs) is ordered in front of whatever the current stream does next.
        params (the optimised parameters): checks that every gradient that was handed to autograd ahead of its producer stream was ADOPTED
        as a parameter's .grad — not cloned, not accumulated into an existing .grad (see `deferred`) — and fails loudly otherwise."""
        self.join_side(final=True)
        self.join_branch()
        n, lost = len(self.deferred), 0
        if n and params is not None:
            have = {p.grad.data_ptr() for p in params if p.grad is not None}
            lost = sum(q not in have for q in self.deferred)
        self._reset()
        if lost:
            raise _lib.DpiError("%d of %d gradients written on a side / branch stream were copied or accumulated by autograd before that stream ran "
                                "(zero_grad(set_to_none=False), a gradient hook, retain_grad or a shared parameter?): with the once-per-step join "
                                "(DPI_JOIN_AT=step) .grad must be None when backward starts; use DPI_JOIN_AT=node otherwise" % (lost, n))

    # ---- side streams ----
    def side_stream(self):
        """The side stream of the next weight gradient (round-robin), marked as having work to join."""
        dev = torch.cuda.current_device()
        sts = self._side_streams.get(dev)
        if sts is None:
            sts = self._side_streams[dev] = [torch.cuda.Stream(device=dev) for _ in range(self.N_SIDE)]
        i = self.side_rr % len(sts)
        self.side_rr += 1
        self.side_used.add(i)
        return sts[i]

    def keep(self, x, chain, dy, dw):
        """After a side-stream launch that reads (x, chain, dy) and writes dw, with the once-per-step join: hold the operands until the
        join and note dw as deferred.  NOT dw itself: the parameter's .grad keeps it alive until the next zero_grad, and a second reference
        would make autograd's AccumulateGrad CLONE it on the main stream — before the side stream has written it — instead of adopting it."""
        if self.join_at == "step" and self.in_iteration:
            self.side_keep.append((x, chain, dy))
            self.deferred.append(dw.data_ptr())

    def defer(self, *tensors):
        """Gradients (None entries skipped) written on a branch stream that autograd receives before that stream has run: see `deferred`."""
        if self.join_at == "step" and self.in_iteration:
            self.deferred.extend(t.data_ptr() for t in tensors if t is not None)

    def join_side(self, final=False):
        """End of a fused node's backward (final=False: nothing to do inside an iteration with the once-per-step join) / end of the whole
        backward (final=True): the current stream waits for every side stream that has work."""
        if self.join_at == "step" and self.in_iteration and not final:
            return
        if self.side_used:
            sts = self._side_streams.get(torch.cuda.current_device()) or []
            for i in sorted(self.side_used):
                torch.cuda.current_stream().wait_stream(sts[i])
            self.side_used.clear()
        self.side_keep.clear()

    # ---- branch streams ----
    def branch_on(self):
        """Never under stream capture: the graph path keeps the serial schedule."""
        return (self.branch_streams and self.overlap and self.in_iteration and self.join_at == "step"
                and not torch.cuda.is_current_stream_capturing())

    def branch(self, kind, *tensors):
        """with sched.branch(kind, tensors...): launches go to the branch stream `kind`, ordered after everything queued on the current
        stream so far.  Memory: every tensor listed was allocated from the current (main) stream's pool and is marked with record_stream,
        so the caching allocator does not hand its memory out again before the branch stream's kernels have run; tensors created inside
        the block come from the branch stream's own pool."""
        key = (torch.cuda.current_device(), kind)
        st = self._branch_streams.get(key)
        if st is None:
            st = self._branch_streams[key] = torch.cuda.Stream(device=key[0])
        st.wait_stream(torch.cuda.current_stream())
        for t in tensors:
            if t is not None:
                t.record_stream(st)
        self.branch_open = True
        return torch.cuda.stream(st)

    def join_branch(self, kind=None):
        """The current stream waits for the branch stream `kind` (None: for all of them).  The backward of a level join relies on autograd
        running ready nodes by descending creation order: ops.SkipTapFn, created before the deeper U, runs after the deeper U's backward and
        joins "skip" there — right before the encoder block of the level consumes the gradient the branch stream wrote."""
        if not self.branch_open:
            return
        dev = torch.cuda.current_device()
        for (d, k), st in self._branch_streams.items():
            if d == dev and (kind is None or k == kind):
                torch.cuda.current_stream().wait_stream(st)
        if kind is None:
            self.branch_open = False
