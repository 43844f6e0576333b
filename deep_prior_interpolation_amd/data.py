"""Patch I/O — drop-in for reference data.py: npy loading, NaN -> binary mask, patch extraction with the
2.5-D slab transposes, and overlap-add reassembly from the per-patch result files.

`reconstruct_patches` sorts the result files by patch name (the reference relies on directory order of an
unsorted glob, data.py:99 — SURVEY App. B.7).

Ours, opt-in: --reassembly cover cuts (and re-assembles) one more, edge-flush window on every axis the regular grid leaves a tail on, --blend
taper weights the overlaps (utils/patch_extractor.py); `reconstruct_patches(field="posterior_std")` blends the per-patch spread of a sampler run,
`reconstruct_patches(field="avo_model")` re-assembles the three parameter sections of an --avo_theta run,
`reconstruct_patches(field="wavelet_model")` the section behind the outputs of a --wavelet run,
`reconstruct_patches(field="moveout_model")` the flattened sections of a --moveout run."""
import os
from glob import glob
from typing import List

import numpy as np

from . import utils as u

__all__ = ["extract_patches", "load_trace_offsets", "load_moveout", "reconstruct_patches", "patch_extractor_for", "transpose_patches_25d"]


def patch_extractor_for(in_shape, patch_shape, patch_stride, datadim, imgchannel=None) -> u.PatchExtractor:
    """-1 in --patch_shape means 'whole axis'; in 2.5-D the last patch axis is the channel stack (data.py:8-17)."""
    ndim = len(in_shape)
    shape = [patch_shape[d] if patch_shape[d] != -1 else in_shape[d] for d in range(ndim)]
    if datadim == "2.5d" and imgchannel is not None:
        shape[-1] = imgchannel
    stride = [patch_stride[d] if patch_stride[d] != -1 else shape[d] for d in range(len(shape))]
    return u.PatchExtractor(dim=tuple(shape), stride=tuple(stride))


_get_patch_extractor = patch_extractor_for   # reference name


def reassembly_flags(args):
    """(cover, blend) of a Namespace; args.txt files of older runs and of the reference lack the keys: crop, flat."""
    reassembly, blend = getattr(args, "reassembly", None) or "crop", getattr(args, "blend", None) or "flat"
    if reassembly not in ("crop", "cover") or blend not in ("flat", "taper"):
        raise ValueError("--reassembly must be crop or cover and --blend flat or taper, got %r, %r" % (reassembly, blend))
    return reassembly == "cover", blend


_TO_SLAB = {"xy": (0, 2, 3, 1), "ty": (0, 1, 3, 2)}   # B,T,X,Y -> B,X,Y,T  /  B,T,Y,X
_FROM_SLAB = {"xy": (0, 3, 1, 2), "ty": (0, 1, 3, 2)}


def transpose_patches_25d(in_content, slice="XY", adj=False):
    """Bring the axis that becomes the conv channel to the end (adj=True undoes it); 'tx' is the identity."""
    s = {"xt": "tx", "yt": "ty"}.get(slice.lower(), slice.lower())
    table = _FROM_SLAB if adj else _TO_SLAB
    return in_content.transpose(table[s]) if s in table else in_content


_transpose_patches_25d = transpose_patches_25d


def extract_patches(args) -> List[dict]:
    """List of {'image': patch*gain, 'mask': binary patch, 'name': zero-padded index} (data.py:44-84).  With --trace_offsets (ours) each
    dict gains 'offsets', the (X, Y, 2) window of the file (2-D: (X, 1, 2) with dy = 0) cut at the origin of its image and mask windows.
    With --moveout or --moveout_offset (ours) each dict gains 'moveout': all of t and the patch's x / y window of the table; with
    --moveout_offset also 'moveout_velocity', the law (T,) of the volume or the laws (T, G_window) of the patch's gathers as used, and with
    --moveout_smooth L > 0 'moveout_pick', the picked staircase(s) behind them in the same shape."""
    original = np.load(os.path.join(args.imgdir, args.imgname), allow_pickle=True)
    corrupted = np.load(os.path.join(args.imgdir, args.maskname), allow_pickle=True)
    assert original.shape == corrupted.shape, "Original and Corrupted data must have the same dimension"
    assert original.ndim in [2, 3], "Data volumes have to be 2D or 3D"
    if np.isnan(corrupted).any():
        corrupted = u.bool2bin(corrupted)
    off = load_trace_offsets(args, original.shape)       # --trace_offsets: refused here, before any window is cut, where it cannot be served
    pe = patch_extractor_for(original.shape, args.patch_shape, args.patch_stride, args.datadim, args.imgchannel)
    # --moveout / --moveout_offset: refused here as well, a time-tiled patch included; the scan reads the known traces of the volume
    scan = {}
    scanned = getattr(args, "moveout_offset", None) is not None
    mov = load_moveout(args, original.shape, pe, volume=original * args.gain if scanned else None, mask=corrupted, scan=scan)
    if args.datadim == "2.5d" or (args.datadim == "2d" and pe.ndim == 3):
        final_shape = (-1,) + pe.dim              # last axis = channels
    else:
        final_shape = (-1,) + pe.dim + (1,)
    if reassembly_flags(args)[0]:
        origins = u.window_origins(original.shape, pe.dim, pe.stride, cover=True)
        img = u.extract_at(original, origins, pe.dim).reshape(final_shape)
        msk = u.extract_at(corrupted, origins, pe.dim).reshape(final_shape)
    else:
        img = pe.extract(original).reshape(final_shape)
        msk = pe.extract(corrupted).reshape(final_shape)
    if args.datadim == "2.5d":
        img = transpose_patches_25d(img, args.slice)
        msk = transpose_patches_25d(msk, args.slice)
    offs = _trace_offset_windows(args, off, original.shape, pe)
    movs = _moveout_windows(args, mov, original.shape, pe)
    laws = _velocity_windows(args, scan, original.shape, pe)
    picks = _velocity_windows(args, scan, original.shape, pe, "pick") if scan.get("smooth", 0.0) > 0.0 else None
    width = u.ten_digit(img.shape[0])
    out = []
    for p in range(img.shape[0]):
        m = msk[p]
        if args.adirandel > 0:
            m = u.add_rand_mask(m, args.adirandel)
        out.append({"image": img[p] * args.gain, "mask": m, "name": str(p).zfill(width)})
        if offs is not None:
            out[-1]["offsets"] = offs[p]
        if movs is not None:
            out[-1]["moveout"] = movs[p]
        if laws is not None:
            out[-1]["moveout_velocity"] = laws[p]
        if picks is not None:
            out[-1]["moveout_pick"] = picks[p]
    return out


def load_trace_offsets(args, vol_shape):
    """--trace_offsets: the file as (X, Y, 2) fp32 for a (T, X, Y) volume, (X, 1, 2) with dy = 0 for a (T, X) section; None when the flag is
    off.  A geometry the flag does not serve, a wrong shape, non-finite values and |d| > 0.5 raise ValueError."""
    name = getattr(args, "trace_offsets", None)
    if name is None:
        return None
    if args.datadim == "2d" and len(vol_shape) == 3:
        raise ValueError("--trace_offsets with --datadim 2d needs a (T, X) section: %s is a 3-D volume whose last axis becomes channels, "
                         "across which nothing can be sampled" % (args.imgname,))
    if args.datadim not in ("2d", "3d") or len(vol_shape) != (2 if args.datadim == "2d" else 3):
        raise ValueError("--trace_offsets needs --datadim 3d on a (T, X, Y) volume or --datadim 2d on a (T, X) section, got --datadim %s on "
                         "a volume of shape %s" % (args.datadim, tuple(vol_shape)))
    off = np.load(os.path.join(args.imgdir, name), allow_pickle=False)
    if len(vol_shape) == 2:
        want = "(%d,) or (%d, 1)" % (vol_shape[1], vol_shape[1])
        ok = off.shape in ((vol_shape[1],), (vol_shape[1], 1))
    else:
        want = "(%d, %d, 2)" % (vol_shape[1], vol_shape[2])
        ok = off.shape == (vol_shape[1], vol_shape[2], 2)
    if not ok or off.dtype.kind not in "fiu":
        raise ValueError("--trace_offsets %s holds %s %s for a volume of shape %s: expected real numbers of shape %s"
                         % (name, off.dtype, tuple(off.shape), tuple(vol_shape), want))
    off = off.astype(np.float32)
    if len(vol_shape) == 2:
        off = np.stack([off.reshape(-1, 1), np.zeros((off.size, 1), dtype=np.float32)], axis=-1)
    if not np.all(np.isfinite(off)):
        raise ValueError("--trace_offsets %s holds non-finite values" % name)
    if np.abs(off).max() > 0.5:
        raise ValueError("--trace_offsets %s: offsets are in grid cells and must lie in [-0.5, 0.5] (a trace belongs to the bin it is "
                         "nearest to), got |d| up to %g" % (name, float(np.abs(off).max())))
    return off


def load_moveout(args, vol_shape, pe=None, volume=None, mask=None, scan=None):
    """--moveout: the table of the file as fp32 in the volume's shape — (T, X, Y) for --datadim 3d, (T, X) for --datadim 2d —, checked once
    for the whole volume (operators.check_moveout_table); None when the flag is off.  A geometry the flag does not serve, a wrong shape,
    non-finite values, live values that decrease along t and, with the patch extractor given, a patch that does not span the time axis
    raise ValueError.
    --moveout_offset: the same table, built by operators.scan_table from the known traces of `volume` (gained, the volume's shape) under
    `mask` (non-zero = known) and the offsets of the file, on the current device; `scan`, a dict, receives what scan_table returned.  The
    kernel sums in a fixed order and the picker is float64 numpy in a fixed order: every rank of parallel.py computes the same table
    from the same files, so nothing is communicated."""
    from .parameter import check_moveout_scan
    flags = check_moveout_scan(args)
    if flags is not None:
        return _scan_moveout(args, flags, vol_shape, pe, volume, mask, scan)
    name = getattr(args, "moveout", None)
    if name is None:
        return None
    if args.datadim not in ("2d", "3d") or len(vol_shape) != (2 if args.datadim == "2d" else 3):
        raise ValueError("--moveout needs --datadim 3d on a (T, X, Y) volume or --datadim 2d on a (T, X) section, got --datadim %s on a "
                         "volume of shape %s" % (args.datadim, tuple(vol_shape)))
    if pe is not None and int(pe.dim[0]) != int(vol_shape[0]):
        raise ValueError("--moveout needs patches that span the whole time axis (%d samples), got %d along t from --patch_shape: the "
                         "table can point anywhere along a trace, so a window in t cannot be served" % (vol_shape[0], pe.dim[0]))
    tab = np.load(os.path.join(args.imgdir, name), allow_pickle=False)
    if tab.shape != tuple(vol_shape) or tab.dtype.kind not in "fiu":
        raise ValueError("--moveout %s holds %s %s for a volume of shape %s: expected real numbers of the volume's shape"
                         % (name, tab.dtype, tuple(tab.shape), tuple(vol_shape)))
    from .operators.moveout import check_moveout_table
    try:
        return check_moveout_table(tab, what="the table")[0]
    except ValueError as e:
        raise ValueError("--moveout %s: %s" % (name, e)) from e


def _scan_moveout(args, flags, vol_shape, pe, volume, mask, scan):
    """--moveout_offset: the offsets of the file, checked, -> the scanned table as load_moveout returns a table read from a file."""
    name = flags["file"]
    if args.datadim not in ("2d", "3d") or len(vol_shape) != (2 if args.datadim == "2d" else 3):
        raise ValueError("--moveout_offset needs --datadim 3d on a (T, X, Y) volume or --datadim 2d on a (T, X) section, got --datadim %s "
                         "on a volume of shape %s" % (args.datadim, tuple(vol_shape)))
    if pe is not None and int(pe.dim[0]) != int(vol_shape[0]):
        raise ValueError("--moveout_offset needs patches that span the whole time axis (%d samples), got %d along t from --patch_shape: "
                         "the table can point anywhere along a trace, so a window in t cannot be served" % (vol_shape[0], pe.dim[0]))
    off = np.load(os.path.join(args.imgdir, name), allow_pickle=False)
    want = (tuple(vol_shape[1:]),) if len(vol_shape) == 3 else ((vol_shape[1],), (vol_shape[1], 1))
    if off.shape not in want or off.dtype.kind not in "fiu":
        raise ValueError("--moveout_offset %s holds %s %s for a volume of shape %s: expected real numbers of shape %s"
                         % (name, off.dtype, tuple(off.shape), tuple(vol_shape), " or ".join(str(w) for w in want)))
    off = off.astype(np.float64).reshape(vol_shape[1:])
    if not np.all(np.isfinite(off)):
        raise ValueError("--moveout_offset %s holds non-finite values" % name)
    if volume is None or mask is None:
        raise ValueError("--moveout_offset %s: the scan needs the volume and its mask (data.extract_patches passes them)" % name)
    from .operators.moveout import check_moveout_table
    from .operators.velocity import scan_table
    known = np.asarray(mask) != 0
    try:
        res = scan_table(np.where(known, np.asarray(volume), 0.0), known, off, flags["vmin"], flags["vmax"], flags["nv"], gather=flags["gather"],
                         window=flags["window"], min_fold=flags["min_fold"], max_step=flags["max_step"], stretch_mute=flags["stretch_mute"],
                         smooth=flags.get("smooth", 0.0), table=flags.get("table", "host"))
    except ValueError as e:
        raise ValueError("--moveout_offset %s: %s" % (name, e)) from e
    if scan is not None:
        scan.update(res, gather=flags["gather"], smooth=flags.get("smooth", 0.0))
    return check_moveout_table(res["table"], what="the table")[0]


def _velocity_windows(args, scan, vol_shape, pe, key="velocity"):
    """The laws that belong to each image window (--moveout_offset), in the order of the image windows; None without a scan.  `key`:
    "velocity" = the laws as used, "pick" = the picked staircases behind them (--moveout_smooth)."""
    if not scan:
        return None
    from .operators.velocity import velocity_windows
    origins = u.window_origins(vol_shape, pe.dim, pe.stride, cover=reassembly_flags(args)[0])
    return velocity_windows(scan[key], scan["gather"], origins, pe.dim)


def _moveout_windows(args, tab, vol_shape, pe):
    """The table windows (num_patches, T, X[, Y]) in the order of the image windows: all of t, the (x, y) part of the same origins."""
    if tab is None:
        return None
    origins = u.window_origins(vol_shape, pe.dim, pe.stride, cover=reassembly_flags(args)[0])
    if len(vol_shape) == 2:
        return np.stack([tab[:, int(o[1]):int(o[1]) + int(pe.dim[1])] for o in origins])
    return np.stack([tab[:, int(o[1]):int(o[1]) + int(pe.dim[1]), int(o[2]):int(o[2]) + int(pe.dim[2])] for o in origins])


def _trace_offset_windows(args, off, vol_shape, pe):
    """The offset windows (num_patches, X, Y, 2) in the order of the image windows: the (x, y) part of the same origins, crop or cover."""
    if off is None:
        return None
    origins = u.window_origins(vol_shape, pe.dim, pe.stride, cover=reassembly_flags(args)[0])
    if len(vol_shape) == 2:
        return np.stack([off[int(o[1]):int(o[1]) + int(pe.dim[1])] for o in origins])
    return np.stack([off[int(o[1]):int(o[1]) + int(pe.dim[1]), int(o[2]):int(o[2]) + int(pe.dim[2])] for o in origins])


def _reconstruct_avo_model(args, results_root):
    """The windows of the (T, X, ntheta) volume with the angle axis swapped for the three parameter sections: the same origins and, under
    --blend taper, the same ramps along t and x (the last axis is one whole window either way)."""
    cover, blend = reassembly_flags(args)
    inputs = np.load(os.path.join(args.imgdir, args.imgname), allow_pickle=True)
    pe = patch_extractor_for(inputs.shape, args.patch_shape, args.patch_stride, args.datadim, args.imgchannel)
    if args.datadim != "2.5d" or args.slice != "tx" or inputs.ndim != 3 or pe.dim[-1] != inputs.shape[-1]:
        raise ValueError("field avo_model belongs to an --avo_theta run: --datadim 2.5d --slice tx on a (T, X, ntheta) volume whose angle "
                         "axis is one window (--imgchannel %r against %r angles)" % (args.imgchannel, inputs.shape[-1]))
    files = sorted((p for p in glob(os.path.join(results_root, args.outdir) + "/*.npy") if "output" not in os.path.basename(p)),
                   key=lambda p: os.path.basename(p))
    outs = []
    for path in files:
        rec = np.load(path, allow_pickle=True).item()
        if "avo_theta" not in rec:
            raise ValueError("%s holds no avo_model: not the result of an --avo_theta run" % path)
        v = rec.get("avo_model")
        outs.append(np.asarray(v) if v is not None else np.zeros(tuple(pe.dim[:-1]) + (3,), dtype=np.float32))
    in_size, dim, stride = tuple(inputs.shape[:-1]) + (3,), tuple(pe.dim[:-1]) + (3,), tuple(pe.stride[:-1]) + (3,)
    origins = u.window_origins(in_size, dim, stride, cover=cover)
    if len(outs) != len(origins):
        raise ValueError("%d result files for %d windows" % (len(outs), len(origins)))
    return u.reassemble(np.asarray(outs).reshape((-1,) + dim), origins, u.reassembled_shape(in_size, dim, stride, cover), dim, stride,
                        blend) / args.gain


def reconstruct_patches(args, return_history=False, verbose=False, results_root="./results", field="output"):
    """Re-assemble the volume from ./results/<outdir>/<name>_run.npy (data.py:87-130).

    field = "posterior_std" (a sampler run, --optimizer sgld | psgld) blends the per-patch spread instead:
    sqrt(sum(w sigma^2) / sum(w)) / |gain|, a patch without one (skipped, or fewer than two samples) counting as 0.  --reassembly cover
    returns the input's shape, --blend taper weights the overlaps; with the defaults and field = "output" nothing differs from before.
    field = "avo_model" (an --avo_theta run) re-assembles the per-patch parameter sections (T, X, 3) into (T', X', 3) with the same windows
    and weights along t and x, divided by gain (the model is linear in the data); a skipped patch counts as zeros.
    field = "wavelet_model" (a --wavelet run) re-assembles the per-patch sections behind the outputs exactly like the outputs: same windows,
    same weights, divided by gain; a patch without one (skipped) counts as zeros.  field = "moveout_model" (a --moveout run) does the
    same for the flattened sections behind the outputs."""
    if field not in ("output", "posterior_std", "avo_model", "wavelet_model", "moveout_model"):
        raise ValueError("field must be output, posterior_std, avo_model, wavelet_model or moveout_model, got %r" % (field,))
    if field == "avo_model":
        return _reconstruct_avo_model(args, results_root)
    cover, blend = reassembly_flags(args)
    inputs = np.load(os.path.join(args.imgdir, args.imgname), allow_pickle=True)
    pe = patch_extractor_for(inputs.shape, args.patch_shape, args.patch_stride, args.datadim, args.imgchannel)
    pe.extract(inputs)
    pa_shape = u.patch_array_shape(inputs.shape, pe.dim, pe.stride)
    files = [p for p in glob(os.path.join(results_root, args.outdir) + "/*.npy")
             if "output" not in os.path.basename(p)]
    files.sort(key=lambda p: os.path.basename(p))
    outs, elapsed, history, dev = [], [], [], "?"
    for path in files:
        rec = np.load(path, allow_pickle=True).item()
        if field == "wavelet_model" and "wavelet" not in rec:
            raise ValueError("%s holds no wavelet_model: not the result of a --wavelet run" % path)
        if field == "moveout_model" and "moveout" not in rec:
            raise ValueError("%s holds no moveout_model: not the result of a --moveout run" % path)
        v = rec["output"] if field == "output" else rec.get(field)
        outs.append(np.asarray(v) if v is not None else np.zeros_like(np.asarray(rec["output"])))
        elapsed.append(rec.get("elapsed", rec.get("elapsed time")))
        history.append(rec["history"])
        dev = rec.get("device", dev)
    # skipped (all-masked) patches are stored with a trailing singleton channel (main.py:283)
    outs = [o[..., 0] if (o.ndim == len(pe.dim) + 1 and o.shape[-1] == 1 and args.datadim != "2.5d") else o for o in outs]
    patches_out = np.asarray(outs)
    if args.datadim == "2.5d":
        patches_out = transpose_patches_25d(patches_out, args.slice, adj=True)
    linear = field in ("output", "wavelet_model", "moveout_model")          # blended like the data and divided by gain; else a spread
    if not cover and blend == "flat" and linear:
        outputs = pe.reconstruct(patches_out.reshape(pa_shape)) / args.gain
    else:
        origins = u.window_origins(inputs.shape, pe.dim, pe.stride, cover=cover)
        outputs = u.reassemble(patches_out.reshape((-1,) + pe.dim), origins, u.reassembled_shape(inputs.shape, pe.dim, pe.stride, cover),
                               pe.dim, pe.stride, blend, spread=not linear) / (args.gain if linear else abs(args.gain))
    if verbose:
        print("\n%d patches; total elapsed time on %s: %s"
              % (len(history), dev, u.sec2time(sum(u.time2sec(e) for e in elapsed if e))))
    return (outputs, history) if return_history else outputs
