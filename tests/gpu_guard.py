"""Guard bands around the buffers a kernel test hands to the library (a plain module: no fixtures, no GPU needed to import it).

One allocation laid out as [front band | payload | back band].  The bands hold a fixed, position-dependent bit pattern, the payload NaN
(so an element a launch was meant to write and did not stays visible) or the caller's data.  `check()` compares both bands as integers,
bit for bit, and names the first changed element relative to the payload: -1 is the element in front of it, `n` the first one behind it.

    g = guard(n, torch.float32, "cuda")                  # g.payload: n floats of NaN, at a 256-byte-aligned address
    g = guard(n, torch.bfloat16, "cuda", offset=1)       # ... moved by one element: the caller chooses the address modulo 16
    g = guard_slice(C, V, torch.float32, "cuda")         # g.payload: channels [c0, c0 + C) of a channel-planar [c_total][V] buffer whose
                                                         # other channels are the bands — what a zero-copy concat hands a layer
    launch(..., g.payload.data_ptr(), ...)
    g.check("y")
"""
import torch

BAND = 256                                  # elements per band, at least
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def _pattern(n, int_dtype, device):
    """Band contents: a different value at every position (so a band element copied to another band position shows), never 0 and never
    the bits of a small number.  Built in int64 and narrowed; the wrap-around of the narrowing is part of the pattern."""
    i = torch.arange(n, dtype=torch.int64, device=device)
    v = i * 40503 + 0x5AC3A53C5AC3
    if int_dtype == torch.int64:
        return v * 2654435761 + 0x3C5AC3A5
    bits = 8 * torch.empty((), dtype=int_dtype).element_size()
    v = v & ((1 << bits) - 1)
    v = torch.where(v >= (1 << (bits - 1)), v - (1 << bits), v)
    return v.to(int_dtype)


class Guarded:
    """The payload view and the two bands around it; see the module docstring."""

    def __init__(self, raw, start, n, dtype, shape):
        self.raw, self.start, self.n, self.dtype = raw, start, n, dtype
        self.expect = raw.clone()                                   # the pattern as written (payload positions are ignored)
        self.payload = raw[start:start + n].view(dtype).view(shape)

    def check(self, what="buffer"):
        """Raises AssertionError when an element of either band changed; the message gives its offset relative to the payload."""
        for lo, hi, base in ((0, self.start, -self.start), (self.start + self.n, self.raw.numel(), self.n - (self.start + self.n))):
            bad = (self.raw[lo:hi] != self.expect[lo:hi]).nonzero()
            if bad.numel():
                i = lo + int(bad[0])
                raise AssertionError("%s: guard band changed at payload offset %d (%d of %d band elements differ; bits %#x, expected %#x)" % (
                    what, i + base, int(bad.numel()), hi - lo, int(self.raw[i]), int(self.expect[i])))

    def bits(self):
        """A copy of the payload's bits (to assert that a refused launch left it alone)."""
        return self.raw[self.start:self.start + self.n].clone()

    def untouched(self, bits):
        return bool(torch.equal(self.raw[self.start:self.start + self.n], bits))


def _make(front, n, back, dtype, device, fill, shape, align_to=None):
    if dtype not in _INT:
        raise ValueError("guard: dtype must be float32, bfloat16 or float64, got %s" % dtype)
    size = torch.empty((), dtype=dtype).element_size()
    slack = 256 // size if align_to is not None else 0
    raw = _pattern(front + n + back + slack, _INT[dtype], device)
    if align_to is not None:       # grow the front band until element `front - align_to` of the allocation sits on a 256-byte boundary
        front += (-(raw.data_ptr() + (front - align_to) * size) % 256) // size
    g = Guarded(raw, front, n, dtype, shape)
    if fill is None:
        g.payload.fill_(float("nan"))
    else:
        g.payload.copy_(fill.reshape(shape).to(device=device, dtype=dtype))
    return g


def guard(n, dtype, device, fill=None, offset=0, band=BAND, shape=None):
    """[band + offset | n | band] elements of `dtype`; the payload starts `offset` elements behind a 256-byte-aligned address.
    fill = None: NaN, else a tensor of n elements to copy in."""
    assert n > 0 and band >= BAND and offset >= 0
    g = _make(band + offset, n, band, dtype, device, fill, (n,) if shape is None else shape, align_to=offset)
    assert (g.payload.data_ptr() - offset * g.payload.element_size()) % 256 == 0
    return g


def guard_slice(C, V, dtype, device, fill=None, c0=None, band=BAND):
    """Channels [c0, c0 + C) of a channel-planar [c_total][V] buffer; the channels in front and behind (at least `band` elements each,
    at least one channel) are the bands.  With an odd V the slice starts at an element-aligned address only: 4 bytes for fp32, 2 for bf16."""
    assert C > 0 and V > 0
    lead = max(1, -(-band // V)) if c0 is None else c0
    assert lead >= 1 and lead * V >= band
    g = _make(lead * V, C * V, lead * V, dtype, device, fill, (C, V), align_to=lead * V)      # channel 0 of the buffer is 256-byte aligned
    g.c0, g.c_total = lead, 2 * lead + C
    return g
