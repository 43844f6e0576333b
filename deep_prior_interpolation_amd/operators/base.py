"""Operator algebra (reference operators/base.py:10-67): Chain, Hessian, dottest."""
import torch

from .. import _lib

__all__ = ["Chain", "dottest", "Hessian", "LinearOpFn", "LinearOperator"]


class LinearOpFn(torch.autograd.Function):
    """y = A x for a linear operator object with `_matvec(x, adjoint)`; backward = A^T dy (and A dy for the adjoint call)."""

    @staticmethod
    def forward(ctx, x, op, adjoint):
        if not x.is_cuda or x.dtype != torch.float32:
            raise _lib.DpiError("operators run on fp32 GPU tensors (no CPU path)")
        ctx.op, ctx.adjoint = op, bool(adjoint)
        return op._matvec(x.contiguous(), bool(adjoint))

    @staticmethod
    def backward(ctx, dy):
        return ctx.op._matvec(dy.contiguous(), not ctx.adjoint), None, None


class LinearOperator(torch.nn.Module):
    """What the operators of this package share.  A subclass writes `_matvec(x, adjoint)`, the kernel launch (the name stays clear of
    nn.Module._apply(fn), which .to() / .float() / .cpu() call: those return the operator and move nothing); `forward` / `adjoint` run it
    through LinearOpFn, so both are differentiable.  One that keeps host arrays also writes `_to_device(device, *key)`, which builds its
    device tensors: `upload(device, *key)` calls it once per device (and key) and keeps the result, so an upload ahead of a graph capture
    leaves nothing for the captured iteration to copy."""

    def __init__(self):
        super().__init__()
        self._dev = {}

    def forward(self, x):
        return LinearOpFn.apply(x, self, False)

    def adjoint(self, y):
        return LinearOpFn.apply(y, self, True)

    def upload(self, device, *key):
        """The operator's tensors on `device`, copied there at the first call for it."""
        k = (str(torch.device(device)),) + key if key else str(torch.device(device))
        t = self._dev.get(k)
        if t is None:
            t = self._dev[k] = self._to_device(device, *key)
        return t

    def _check_patch(self, x, exc, ndim_msg, ndims=(4, 5), nonempty=False):
        """x is one patch (1, C, T, X[, Y]) with `ndims` axes, raised as the subclass's `exc`; `ndim_msg` takes x.ndim."""
        name = type(self).__name__
        if x.ndim not in ndims:
            raise exc(ndim_msg % x.ndim)
        if x.shape[0] != 1:
            raise exc("%s works on one patch at a time: batch size %d" % (name, x.shape[0]))
        if nonempty and x.numel() < 1:
            raise exc("%s: empty tensor %s" % (name, tuple(x.shape)))


class Chain(torch.nn.Module):
    """ops[-1](...ops[0](x)); adjoint applies the adjoints in reverse order (base.py:10-37)."""

    def __init__(self, ops: list):
        super().__init__()
        assert len(ops) >= 1
        self.ops = ops

    def forward(self, x):
        for op in self.ops:
            x = op(x)
        return x

    def adjoint(self, x):
        for op in self.ops[::-1]:
            x = op.adjoint(x)
        return x

    def __getitem__(self, item):
        return self.ops[item]


class Hessian(torch.nn.Module):
    """A^T A (base.py:40-50); self-adjoint."""

    def __init__(self, op):
        super().__init__()
        self.op = op

    def forward(self, x):
        return self.op.adjoint(self.op.forward(x))

    def adjoint(self, x):
        return self.forward(x)


def dottest(op, domain_tensor, range_tensor, verbose=True, generator=None):
    """Adjoint dot-product test <A d1, r1> = <d1, A^T r1> on random vectors of the given shapes (base.py:53-67).
    Runs on the device of `domain_tensor`; returns (absolute error, relative error) besides printing them like the reference."""
    dev = domain_tensor.device
    d1 = torch.randn(domain_tensor.shape, generator=generator).to(dev)
    r1 = torch.randn(range_tensor.shape, generator=generator).to(dev)
    r2 = op.forward(d1)
    d2 = op.adjoint(r1)
    d_ = torch.vdot(d1.double().view(-1), d2.double().view(-1))
    r_ = torch.vdot(r1.double().view(-1), r2.double().view(-1))
    err_abs = d_ - r_
    err_rel = err_abs / d_
    if verbose:
        print("Absolute error: %.6e" % abs(err_abs.item()))
        print("Relative error: %.6e \n" % abs(err_rel.item()))
    return abs(err_abs.item()), abs(err_rel.item())
