"""Records tests/golden/avo.npz from a checkout of the reference (polimi-ispl/deep_prior_interpolation): its operators/avo.py is loaded
by file path and run on the CPU; the file holds recorded arrays only.

    python tools/record_avo_golden.py /path/to/reference [--out tests/golden/avo.npz]

Coefficients (`coef/NN/...`): every combination of
    angles [0,10,20,30,40], [5,15,25], [0,7,...,49], [0,60,75]  x  akirich, fatti  x  vsvp 0.5, linspace(0.4, 0.6, nt0)  x  nt0 37, 8
with the reference's fp32 G (ntheta, 3, nt0), its distance from the float64 formula (`gap`, relative to max|G|) and the range of
cond(G_t) over t (`cond_min`, `cond_max`).
Vectors (`vec/NN/...`): the 16 combinations of angles x linearisation x vsvp, on (nt0 37, one spatial axis of 19) where the three indices
sum to an even number and on (nt0 8, two spatial axes 7 x 9) elsewhere — every pair of choices meets both geometries, and the file stays
well under the size a committed fixture may have.  Per case a seeded x (1, 3, nt0, *spat) and y (1, ntheta, nt0, *spat), forward(x) and
adjoint(y) of the reference, and the index `coef` of its coefficient case.
Top level: `gap_max`, `cond_min`, `cond_max` over all coefficient cases."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ANGLES = [[0, 10, 20, 30, 40], [5, 15, 25], list(range(0, 50, 7)), [0, 60, 75]]
LINS = ["akirich", "fatti"]
GEOMETRIES = [(37, (19,)), (8, (7, 9))]


def vsvp_of(kind, nt0):
    return 0.5 if kind == 0 else torch.linspace(0.4, 0.6, nt0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("reference", help="path of the reference checkout")
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "avo.npz"))
    a = p.parse_args()
    spec = importlib.util.spec_from_file_location("reference_avo", os.path.join(a.reference, "operators", "avo.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    from deep_prior_interpolation_amd.operators.avo import avo_coefficients

    out, coef_index = {}, {}
    gaps, conds = [], []
    n = 0
    for ia, angles in enumerate(ANGLES):
        for il, lin in enumerate(LINS):
            for iv in (0, 1):
                for ig, (nt0, _) in enumerate(GEOMETRIES):
                    vsvp = vsvp_of(iv, nt0)
                    op = ref.AVOLinearModelling(torch.tensor(angles, dtype=torch.float32), vsvp=vsvp, nt0=nt0, spatdims=None, linearization=lin)
                    G = op.G.numpy().astype(np.float32)
                    assert G.shape == (len(angles), 3, nt0), G.shape
                    G64 = avo_coefficients(angles, vsvp, nt0, lin)
                    gap = float(np.abs(G.astype(np.float64) - G64).max() / np.abs(G64).max())
                    cond = np.array([np.linalg.cond(G[:, :, t].astype(np.float64)) for t in range(nt0)])
                    k = "coef/%02d/" % n
                    out[k + "G"] = G
                    out[k + "theta"] = np.asarray(angles, dtype=np.float64)
                    out[k + "vsvp"] = np.atleast_1d(np.asarray(vsvp.numpy() if torch.is_tensor(vsvp) else vsvp, dtype=np.float32))
                    out[k + "lin"] = np.array(lin)
                    out[k + "nt0"] = np.array(nt0)
                    out[k + "gap"] = np.array(gap)
                    out[k + "cond_min"], out[k + "cond_max"] = np.array(cond.min()), np.array(cond.max())
                    gaps.append(gap)
                    conds += [cond.min(), cond.max()]
                    coef_index[(ia, il, iv, ig)] = n
                    n += 1
    m = 0
    for ia, angles in enumerate(ANGLES):
        for il, lin in enumerate(LINS):
            for iv in (0, 1):
                ig = (ia + il + iv) % 2
                nt0, spat = GEOMETRIES[ig]
                op = ref.AVOLinearModelling(torch.tensor(angles, dtype=torch.float32), vsvp=vsvp_of(iv, nt0), nt0=nt0, spatdims=spat,
                                            linearization=lin)
                gen = torch.Generator().manual_seed(1000 + m)
                x = torch.randn((1, 3, nt0) + spat, generator=gen)
                y = torch.randn((1, len(angles), nt0) + spat, generator=gen)
                k = "vec/%02d/" % m
                out[k + "coef"] = np.array(coef_index[(ia, il, iv, ig)])
                out[k + "x"], out[k + "y"] = x.numpy(), y.numpy()
                out[k + "fwd"] = op.forward(x).numpy().astype(np.float32)
                out[k + "adj"] = op.adjoint(y).numpy().astype(np.float32)
                assert out[k + "fwd"].shape == y.shape and out[k + "adj"].shape == x.shape
                m += 1
    out["gap_max"] = np.array(max(gaps))
    out["cond_min"], out["cond_max"] = np.array(min(conds)), np.array(max(conds))
    np.savez(a.out, **out)
    print("%d coefficient cases, %d vector cases; fp32-vs-float64 gap of G at most %.3g of max|G|; cond(G_t) from %.3g to %.3g; %d bytes"
          % (n, m, max(gaps), min(conds), max(conds), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
