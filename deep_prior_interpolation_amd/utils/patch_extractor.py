"""N-D sliding-window patch extraction and overlap-add reassembly
(drop-in for the part of reference utils/patch_extractor.py that data.py uses: rectangular taper,
C-order over the window grid, no scoring / shuffling / tapering options).

Window w = (w_0..w_{n-1}) starts at w_k * stride_k; the grid has (in_k - dim_k)//stride_k + 1 windows per
axis; reassembly averages overlapping samples (hit-count normalisation).

Ours, opt-in (--reassembly cover, --blend taper; the functions below `window_origins`): the regular grid drops the tail of every axis
where (n - d) % s != 0, so `cover` adds one edge-flush window at origin n - d there; `taper` replaces the box window of the average by
sin^2 ramps on the sides of a window that have a neighbour (a side on the volume edge stays 1); a spread field (a per-patch standard
deviation) is blended as sqrt(sum(w sigma^2) / sum(w)).  This float64 numpy code DEFINES that arithmetic: the device kernels
(dpi_overlap_add_weighted / dpi_overlap_finalize_weighted) are tested against a restatement of it."""
import numpy as np

__all__ = ["PatchExtractor", "count_patches", "patch_array_shape", "in_content_cropped_shape", "window_origins", "axis_origins",
           "reassembled_shape", "extract_at", "taper_length", "taper_ramp", "axis_window", "patch_window", "taper_sides", "reassemble"]


def _grid(in_size, patch_size, patch_stride):
    return tuple((int(n) - int(d)) // int(s) + 1 for n, d, s in zip(in_size, patch_size, patch_stride))


def count_patches(in_size, patch_size, patch_stride):
    return int(np.prod(_grid(in_size, patch_size, patch_stride)))


def patch_array_shape(in_size, patch_size, patch_stride):
    return _grid(in_size, patch_size, patch_stride) + tuple(patch_size)


def in_content_cropped_shape(in_size, patch_size, patch_stride):
    assert len(in_size) == len(patch_size) == len(patch_stride)
    return tuple((g - 1) * s + d for g, s, d in zip(_grid(in_size, patch_size, patch_stride), patch_stride, patch_size))


def axis_origins(n, d, s, cover=False, axis=0):
    """Window origins along one axis: the regular grid 0, s, 2s, ... and, with cover, one more window flush with the end (origin n - d)
    where the grid leaves a tail, i.e. where (n - d) % s != 0."""
    n, d, s = int(n), int(d), int(s)
    if cover and n < d:
        raise ValueError("--reassembly cover: axis %d of the volume has %d samples, fewer than the patch's %d" % (axis, n, d))
    org = [k * s for k in range((n - d) // s + 1)]
    if cover and (n - d) % s != 0:
        org.append(n - d)
    return org


def window_origins(in_size, patch_size, patch_stride, cover=False):
    """Origins of all windows in C order of the window grid: array (num_patches, ndim).  cover=True: C order of the per-axis origin
    lists of axis_origins (the edge-flush window is the last one of its axis)."""
    if cover:
        per_axis = [axis_origins(n, d, s, True, k) for k, (n, d, s) in enumerate(zip(in_size, patch_size, patch_stride))]
        return np.stack(np.meshgrid(*[np.asarray(o) for o in per_axis], indexing="ij"), axis=-1).reshape(-1, len(per_axis))
    grid = _grid(in_size, patch_size, patch_stride)
    idx = np.stack(np.meshgrid(*[np.arange(g) for g in grid], indexing="ij"), axis=-1).reshape(-1, len(grid))
    return idx * np.asarray(patch_stride)[None, :]


def reassembled_shape(in_size, patch_size, patch_stride, cover=False):
    """Shape of the re-assembled volume: the input's own under cover, else the part the regular grid reaches."""
    if cover:
        window_origins(in_size, patch_size, patch_stride, True)       # raises for an axis shorter than the patch
        return tuple(int(n) for n in in_size)
    return in_content_cropped_shape(in_size, patch_size, patch_stride)


def extract_at(in_content, origins, patch_size):
    """The windows of `patch_size` at `origins`, stacked: array (num_patches,) + patch_size."""
    return np.stack([in_content[tuple(slice(int(o), int(o) + int(d)) for o, d in zip(org, patch_size))] for org in origins])


def taper_length(d, s):
    """Ramp length of a window of d samples on a grid of stride s: the overlap d - s, at most half the window."""
    return max(0, min(int(d) - int(s), int(d) // 2))


def taper_ramp(d, s):
    """r[i] = sin^2(pi (i + 1/2) / (2 L)), i = 0..L-1 (float64, strictly inside (0, 1)): r[i] + r[L-1-i] = 1, so on the regular grid with
    s >= d/2 the falling ramp of a window and the rising ramp of its neighbour sum to exactly 1 over their overlap."""
    L = taper_length(d, s)
    return np.sin(np.pi * (np.arange(L) + 0.5) / (2.0 * L)) ** 2 if L > 0 else np.zeros(0)


def taper_sides(n, d, origin):
    """(low, high): which sides of the window at `origin` have a neighbour, i.e. do not touch the edge of the n-sample axis."""
    return int(origin) > 0, int(origin) + int(d) < int(n)


def axis_window(n, d, s, origin, taper=True):
    """Weights (d,) of the window at `origin` along an axis of n samples: the ramp rising on the low side if origin > 0, mirrored on the
    high side if origin + d < n, 1 elsewhere; all ones without taper or with L = 0."""
    w = np.ones(int(d))
    r = taper_ramp(d, s) if taper else np.zeros(0)
    if len(r):
        lo, hi = taper_sides(n, d, origin)
        if lo:
            w[:len(r)] *= r
        if hi:
            w[int(d) - len(r):] *= r[::-1]
    return w


def patch_window(in_size, patch_size, patch_stride, origin, taper=True):
    """The N-D window of the patch at `origin`: the outer product of its per-axis windows, array of shape patch_size."""
    w = np.ones(())
    for n, d, s, o in zip(in_size, patch_size, patch_stride, origin):
        w = np.multiply.outer(w, axis_window(n, d, s, o, taper))
    return w


def reassemble(patches, origins, out_shape, patch_size, patch_stride, blend="flat", spread=False):
    """Weighted overlap-add of `patches` (num_patches,) + patch_size at `origins` into a volume of `out_shape`:
    mean = sum(w p) / sum(w), or for a spread field (spread=True: a standard deviation per sample) sqrt(sum(w p^2) / sum(w)) — the
    window-weighted mean of the variances, which cannot cancel (E[x^2] - E[x]^2 does, in fp32).  blend = "flat": w = 1, the sums run in
    the order of PatchExtractor.reconstruct and the mean has its bits; "taper": patch_window.  A sample no window reaches gives 0."""
    if blend not in ("flat", "taper"):
        raise ValueError("blend must be flat or taper, got %r" % (blend,))
    patches = np.asarray(patches)
    num = np.zeros(tuple(out_shape))
    den = np.zeros(tuple(out_shape))
    for p, org in zip(patches, origins):
        sl = tuple(slice(int(o), int(o) + int(d)) for o, d in zip(org, patch_size))
        v = p.astype(np.float64) ** 2 if spread else p
        if blend == "taper":
            w = patch_window(out_shape, patch_size, patch_stride, org, True)
            num[sl] += w * v
            den[sl] += w
        else:
            num[sl] += v
            den[sl] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(den > 0, num / den, 0.0)
    return (np.sqrt(out) if spread else out).astype(patches.dtype)


class PatchExtractor:
    def __init__(self, dim, offset=None, stride=None, tapering="rect", padding=None, **unsupported):
        if not isinstance(dim, tuple):
            raise ValueError("dim must be a tuple")
        for k, v in unsupported.items():
            if v is not None:
                raise NotImplementedError("PatchExtractor option %s is outside the hot-path scope" % k)
        if tapering != "rect" or padding is not None:
            raise NotImplementedError("only rectangular tapering without padding is supported")
        self.dim = dim
        self.ndim = len(dim)
        self.offset = tuple([0] * self.ndim) if offset is None else offset
        self.stride = dim if stride is None else stride
        if not isinstance(self.stride, tuple) or len(self.stride) != self.ndim:
            raise ValueError("stride must a tuple of length {:d}".format(self.ndim))
        if not isinstance(self.offset, tuple) or len(self.offset) != self.ndim:
            raise ValueError("offset must a tuple of length {:d}".format(self.ndim))
        self.tapering = "rect"
        self.in_content_original_shape = None
        self.in_content_cropped_shape = None
        self.patch_array_shape = None

    def extract(self, in_content):
        if not isinstance(in_content, np.ndarray):
            raise ValueError("in_content must be of type: " + str(np.ndarray))
        if in_content.ndim != self.ndim:
            raise ValueError("in_content shape must a tuple of length {:d}".format(self.ndim))
        self.in_content_original_shape = in_content.shape
        in_content = in_content[tuple(slice(o, None) for o in self.offset)]
        view = np.lib.stride_tricks.sliding_window_view(in_content, self.dim)
        view = view[tuple(slice(None, None, s) for s in self.stride)]
        patch_array = np.ascontiguousarray(view)
        self.in_content_cropped_shape = tuple((g - 1) * s + d for g, s, d in
                                              zip(patch_array.shape[:self.ndim], self.stride, self.dim))
        self.patch_array_shape = patch_array.shape
        return patch_array

    def reconstruct(self, patch_array):
        if not isinstance(patch_array, np.ndarray):
            raise ValueError("patch_array must be of type: " + str(np.ndarray))
        ndim = patch_array.ndim // 2
        grid = patch_array.shape[:ndim]
        image_shape = tuple((g - 1) * s + d for g, s, d in zip(grid, self.stride, self.dim))
        if self.in_content_cropped_shape is not None and image_shape != tuple(self.in_content_cropped_shape):
            raise ValueError("There is something wrong with the dimensions!")
        recon = np.zeros(image_shape)
        hits = np.zeros(image_shape)
        for idx in np.ndindex(*grid):
            sl = tuple(slice(i * s, i * s + d) for i, s, d in zip(idx, self.stride, self.dim))
            recon[sl] += patch_array[idx]
            hits[sl] += 1
        recon /= hits
        return recon.astype(patch_array.dtype)
